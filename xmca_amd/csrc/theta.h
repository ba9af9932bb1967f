// Theta fore/back-cast fit of every column of a resident T x N float64 field (solve(complexify=True, extend='theta', period=m);
// DESIGN.md 2.11).  One lane per column, so every time step is one coalesced row read.  Two kernels per field:
//   theta_season_kernel   additive seasonal means s_p (centred moving average of length m) and the drift b0 of z = y - s
//   theta_smooth_kernel   simple exponential smoothing of z: alpha by a fixed grid zoom (6 rounds of 33 candidates), the level,
//                         and the coefficients of the forecast in the basis (1, h, [(T + h) mod m == p])
// blockIdx.y = 0 fits the column as it is (forecast), 1 the reversed column (backcast).  Every sum runs in time order inside one
// lane and the candidates are merged in a fixed order through LDS: no atomics, a column's result does not depend on the grid.
// The arithmetic is written without contraction, operation by operation as the numpy restatement of the tests does it.
#pragma once
#include "common.h"

namespace xmca {

constexpr int THETA_ROUNDS = 6;      // grid zoom: rounds ...
constexpr int THETA_CAND = 33;       // ... of this many candidates a_i = lo + (hi - lo) i / 32
constexpr int THETA_GROUPS = 3;      // waves of a workgroup, each carrying ...
constexpr int THETA_PER = 11;        // ... this many candidates of every lane's column as independent recurrences
constexpr int THETA_HEAD = 5;        // rows of a fit before the seasonal means: alpha, b0, level, c_const, c_slope
constexpr double THETA_ALPHA_LO = 1e-4, THETA_ALPHA_HI = 1.0 - 1e-4;
static_assert(THETA_GROUPS * THETA_PER == THETA_CAND, "the waves of a workgroup share the candidates of a round evenly");

// rows of one direction's fit (each N values): alpha, b0, level, then the 2 + m coefficients of the forecast
//   f_h = c_const + c_slope h + s[(T + h) mod m]:  c_const = level + 0.95 b0 (1 - (1 - alpha)^T) / alpha,  c_slope = 0.95 b0,  s_0 .. s_{m-1}
__host__ __device__ static inline int64_t theta_fit_rows(int m) { return THETA_HEAD + m; }

// number of t in [0, x) with t = p (mod m)
__device__ __forceinline__ int theta_phase_count(int x, int p, int m) { return x > p ? (x - 1 - p) / m + 1 : 0; }

__global__ __launch_bounds__(256) void theta_season_kernel(const double* __restrict__ X, int T, int64_t N, int m, double* __restrict__ fit) {
#pragma clang fp contract(off)
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= N) return;
  const bool rev = blockIdx.y == 1;
  double* F = fit + (int64_t)blockIdx.y * theta_fit_rows(m) * N + col;
  double* S = F + (int64_t)THETA_HEAD * N;
  const double* Xc = X + col;
  auto y = [&](int t) { return Xc[(int64_t)(rev ? T - 1 - t : t) * N]; };
  if (m >= 2) {
    const int h = m / 2, t_end = T - h;
    for (int p = 0; p < m; ++p) S[(int64_t)p * N] = 0.0;
    int p = h;                                         // (h < m)
    for (int t = h; t < t_end; ++t) {
      double acc;
      if (m & 1) {
        acc = y(t - h);
#pragma unroll 8
        for (int k = 1; k < m; ++k) acc += y(t - h + k);        // (unrolled: the reads of a window are in flight together)
      } else {
        acc = 0.5 * y(t - h);
#pragma unroll 8
        for (int k = 1; k < m; ++k) acc += y(t - h + k);
        acc += 0.5 * y(t + h);
      }
      S[(int64_t)p * N] += y(t) - acc / (double)m;
      if (++p == m) p = 0;
    }
    double mean = 0.0;
    for (int q = 0; q < m; ++q) {                      // (T >= 2m: every phase has a defined value)
      const int cnt = theta_phase_count(t_end, q, m) - theta_phase_count(h, q, m);
      const double a = S[(int64_t)q * N] / (double)cnt;
      S[(int64_t)q * N] = a;
      mean += a;
    }
    mean = mean / (double)m;
    for (int q = 0; q < m; ++q) S[(int64_t)q * N] -= mean;
  } else {
    S[0] = 0.0;
  }
  // drift: least-squares slope of z on t, sum (t - tbar) z_t / (T (T^2 - 1) / 12)
  const double tbar = 0.5 * (double)(T - 1);
  double num = 0.0;
  int p = 0;
#pragma unroll 8
  for (int t = 0; t < T; ++t) {
    const double z = y(t) - S[(int64_t)p * N];
    num += ((double)t - tbar) * z;
    if (++p == m) p = 0;
  }
  const double n = (double)T;
  F[(int64_t)N] = num / (n * (n * n - 1.0) / 12.0);
}

// blockDim = (64, THETA_GROUPS): lane x takes column blockIdx.x * 64 + x, wave y the candidates y * 11 .. y * 11 + 10 of it
__global__ __launch_bounds__(64 * THETA_GROUPS) void theta_smooth_kernel(const double* __restrict__ X, int T, int64_t N, int m,
                                                                         double* __restrict__ fit) {
#pragma clang fp contract(off)
  __shared__ double s_sse[THETA_GROUPS][64], s_lvl[THETA_GROUPS][64];
  __shared__ int s_idx[THETA_GROUPS][64];
  const int lane = threadIdx.x, g = threadIdx.y;
  const int64_t col_raw = (int64_t)blockIdx.x * 64 + lane;
  const bool live = col_raw < N;
  const int64_t col = live ? col_raw : N - 1;          // (lanes past the field follow the last column and write nothing)
  const bool rev = blockIdx.y == 1;
  double* F = fit + (int64_t)blockIdx.y * theta_fit_rows(m) * N + col;
  const double* S = F + (int64_t)THETA_HEAD * N;
  const double* Xc = X + col;
  auto y = [&](int t) { return Xc[(int64_t)(rev ? T - 1 - t : t) * N]; };
  const double z0 = y(0) - S[0];
  double lo = THETA_ALPHA_LO, hi = THETA_ALPHA_HI, alpha = lo, level = z0;
  for (int round = 0; round < THETA_ROUNDS; ++round) {
    const double width = hi - lo;
    double a[THETA_PER], l[THETA_PER], sse[THETA_PER];
#pragma unroll
    for (int u = 0; u < THETA_PER; ++u) {
      a[u] = lo + width * ((double)(g * THETA_PER + u) / 32.0);
      l[u] = z0;
      sse[u] = 0.0;
    }
    int p = m > 1 ? 1 : 0;
#pragma unroll 8
    for (int t = 1; t < T; ++t) {
      const double z = y(t) - S[(int64_t)p * N];
      if (++p == m) p = 0;
#pragma unroll
      for (int u = 0; u < THETA_PER; ++u) {
        const double e = z - l[u];
        l[u] = l[u] + a[u] * e;
        sse[u] = sse[u] + e * e;
      }
    }
    // lowest SSE, lowest index on ties: inside the lane, then over the waves in their order
    double best = sse[0], best_l = l[0];
    int bi = 0;
#pragma unroll
    for (int u = 1; u < THETA_PER; ++u) {
      const bool better = sse[u] < best;
      best = better ? sse[u] : best;
      best_l = better ? l[u] : best_l;
      bi = better ? u : bi;
    }
    s_sse[g][lane] = best;
    s_lvl[g][lane] = best_l;
    s_idx[g][lane] = g * THETA_PER + bi;
    __syncthreads();
    double win = s_sse[0][lane];
    int j = s_idx[0][lane];
    level = s_lvl[0][lane];
#pragma unroll
    for (int w = 1; w < THETA_GROUPS; ++w) {
      const bool better = s_sse[w][lane] < win;
      win = better ? s_sse[w][lane] : win;
      j = better ? s_idx[w][lane] : j;
      level = better ? s_lvl[w][lane] : level;
    }
    __syncthreads();                                   // (the next round writes the same LDS)
    alpha = lo + width * ((double)j / 32.0);
    const double nlo = lo + width * ((double)(j > 0 ? j - 1 : 0) / 32.0);
    const double nhi = lo + width * ((double)(j < THETA_CAND - 1 ? j + 1 : THETA_CAND - 1) / 32.0);
    lo = nlo;
    hi = nhi;
  }
  if (g != 0 || !live) return;
  const double b0 = F[(int64_t)N];
  const double q = 1.0 - alpha;
  double pw = 1.0;
  for (int k = 0; k < T; ++k) pw = pw * q;
  const double slope = 0.95 * b0;
  F[0] = alpha;
  F[(int64_t)2 * N] = level;
  F[(int64_t)3 * N] = level + slope * ((1.0 - pw) / alpha);
  F[(int64_t)4 * N] = slope;
}

// fit: 2 x (THETA_HEAD + m) x N doubles (forecast, then backcast; rows as above)
static inline void theta_fit(hipStream_t st, const double* X, int64_t T, int64_t N, int m, double* fit) {
  hipLaunchKernelGGL(theta_season_kernel, dim3((unsigned)ceil_div(N, (int64_t)256), 2), dim3(256), 0, st, X, (int)T, N, m, fit);
  XMCA_HIP(hipGetLastError());
  hipLaunchKernelGGL(theta_smooth_kernel, dim3((unsigned)ceil_div(N, (int64_t)64), 2), dim3(64, THETA_GROUPS), 0, st, X, (int)T, N, m, fit);
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
