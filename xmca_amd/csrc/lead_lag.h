// Lead-lag maps: regression and correlation of every column of a T x N field with missing values (NaN) on q <= 8
// gap-free index series at a list of lags, xmca_amd.lagged.lead_lag_maps.  For lag l the pairs of column n are (y[s], x[s + l][n])
// over the steps s in [max(0, -l), min(T, T - l)) at which x[s + l][n] is present: a positive lag means the index leads the field.
// All sums are float64 chains in ascending s that start from +0.0, whatever the type of the field, over x' = x - c_n (c_n the mean
// of the column's present values, against cancellation) and the centred index y'.  Four kernels, none with an atomic, with scratch
// memory or with a mask / widened plane; a gap is recognised on load by v == v.  A call repeats its bits, and the chains of a lag
// are its own: its results do not depend on the other lags of the call nor on their order.
#pragma once
#include <limits>

#include "kernels.h"

namespace xmca {

constexpr int LL_COLS = 256;                     // columns of a workgroup: one lane each (xmca_lead_lag_tile)
constexpr int LL_ROWS = 8;                       // rows of a piece: the loads a lane keeps in flight
constexpr int LL_MAX_Q = 8;                      // most index series
constexpr int LL_MAX_ENTRIES = 1024;             // most lags x index series of a call
constexpr double LL_LIVE = 0x1p-40;              // an entry is live when Cxx > LL_LIVE Sxx and Cyy > LL_LIVE Syy

// lags of a group per number of index series: G (3 + 3 Q) accumulators of a lane, chosen from the register report
__host__ __device__ constexpr int ll_group(int q) { return q == 1 ? 8 : q == 2 ? 6 : q == 3 ? 4 : q <= 5 ? 3 : 2; }
// values per (lag, column) of the moments plane: Sx, Sxx and per index series Sy, Syy, Sxy (the count goes to `pairs`)
__host__ __device__ constexpr int ll_moments(int q) { return 2 + 3 * q; }

// 1. The mean of the present values of every column and their number: one lane per column, one ascending chain from +0.0.
// Bounds: X at rows t < T, columns n < N; cn, n0 at n < N.
template <typename TI>
__global__ __launch_bounds__(LL_COLS) void lead_lag_center_kernel(const TI* __restrict__ X, int T, int64_t N, double* __restrict__ cn,
                                                                  int* __restrict__ n0) {
  constexpr int R = LL_ROWS;
  const int64_t n = (int64_t)blockIdx.x * LL_COLS + threadIdx.x;
  if (n >= N) return;
  const TI* col = X + n;
  double s = 0.0;
  int c = 0;
  for (int t0 = 0; t0 < T; t0 += R) {
    TI v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int t = t0 + i < T ? t0 + i : T - 1;          // (no branch around the load: a row past the record reads the last one)
      v[i] = col[(int64_t)t * N];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const bool present = t0 + i < T && v[i] == v[i];
      s += present ? (double)v[i] : 0.0;
      c += present ? 1 : 0;
    }
  }
  cn[n] = c > 0 ? s / (double)c : 0.0;
  n0[n] = c;
}

// 2. The lag-1 autocorrelation of every column over its present neighbours (dof = 'bretherton'):
// rho = [sum_P x'_t x'_{t+1} / |P|] / [sum_present x'^2 / n0], P the steps t with x[t] and x[t + 1] present; 0 where |P| = 0 or the
// denominator is not positive; clamped to [-1, 1].  One lane per column, one pass, both chains ascending from +0.0.
// Bounds: X at rows t < T, columns n < N; cn, n0, rho at n < N.
template <typename TI>
__global__ __launch_bounds__(LL_COLS) void lag1_gappy_kernel(const TI* __restrict__ X, int T, int64_t N, const double* __restrict__ cn,
                                                             const int* __restrict__ n0, double* __restrict__ rho) {
  constexpr int R = LL_ROWS;
  const int64_t n = (int64_t)blockIdx.x * LL_COLS + threadIdx.x;
  if (n >= N) return;
  const TI* col = X + n;
  const double c = cn[n];
  double sq = 0.0, sp = 0.0, prev = 0.0;          // (prev: x' of the step before, 0 where that is missing - the product vanishes)
  int np = 0;
  bool had = false;
  for (int t0 = 0; t0 < T; t0 += R) {
    TI v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int t = t0 + i < T ? t0 + i : T - 1;
      v[i] = col[(int64_t)t * N];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const bool present = t0 + i < T && v[i] == v[i];
      const double x = present ? (double)v[i] - c : 0.0;
      sq = fma(x, x, sq);
      sp = fma(prev, x, sp);
      np += present && had ? 1 : 0;
      prev = x;
      had = present;
    }
  }
  const double den = sq / (double)n0[n];
  double r = 0.0;
  if (np > 0 && den > 0.0) r = (sp / (double)np) / den;
  rho[n] = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// 3. The moments, the hot path.  A workgroup owns LL_COLS columns x one group of G lags (blockIdx.y; the last group may be partial:
// its spare slots repeat the last lag of the call and are not written).  A lane owns one column and keeps the G (3 + 3 Q)
// accumulators of its group in registers - the count an int, the rest doubles.  It streams the T rows of its column once, in
// unrolled pieces of LL_ROWS rows whose loads are issued together; row t meets lag l with the index row s = t - l.  That row is the
// same for the whole workgroup: the lags sit in scalar registers and y'[s][.] comes through wave-uniform loads.  A pair outside
// the record, or with x missing, adds +0.0 to every chain: x' is selected to 0 and y' enters as one * y with one = pair ? 1 : 0,
// an exact product (the chains start from +0.0 and the index is finite, so the zeros leave their bits alone; a 64-bit select
// per series instead took 256 VGPRs and AGPRs beside them).  No branch surrounds a load: the field row is clamped to T - 1, the
// index row to [0, T).
// Bounds: X at rows [0, T), columns n < N; cn at n < N; Y (T x Q, row-major) at rows [0, T); lags at g < n_lags;
// pairs at (g, n) and mom at (g, k < 2 + 3 Q, n) with g < n_lags, n < N.
template <typename TI, int Q, int G>
__global__ __launch_bounds__(LL_COLS) void lead_lag_moments_kernel(const TI* __restrict__ X, int T, int64_t N, const double* __restrict__ cn,
                                                                   const double* __restrict__ Y, const int* __restrict__ lags, int n_lags,
                                                                   int* __restrict__ pairs, double* __restrict__ mom) {
  constexpr int R = LL_ROWS;
  constexpr int M = ll_moments(Q);
  const int64_t n = (int64_t)blockIdx.x * LL_COLS + threadIdx.x;
  if (n >= N) return;
  const int g0 = (int)blockIdx.y * G;
  int lag[G];
#pragma unroll
  for (int g = 0; g < G; ++g) lag[g] = lags[g0 + g < n_lags ? g0 + g : n_lags - 1];
  int cnt[G];
  double sx[G], sxx[G], sy[G][Q], syy[G][Q], sxy[G][Q];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    cnt[g] = 0;
    sx[g] = sxx[g] = 0.0;
#pragma unroll
    for (int j = 0; j < Q; ++j) sy[g][j] = syy[g][j] = sxy[g][j] = 0.0;
  }
  const TI* col = X + n;
  const double c = cn[n];
  for (int t0 = 0; t0 < T; t0 += R) {
    TI v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int t = t0 + i < T ? t0 + i : T - 1;
      v[i] = col[(int64_t)t * N];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int t = t0 + i;
      const bool present = t < T && v[i] == v[i];
      const double x = present ? (double)v[i] - c : 0.0;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int s = t - lag[g];                              // (uniform over the workgroup)
        const bool inside = s >= 0 && s < T;
        const int sc = s < 0 ? 0 : (s < T ? s : T - 1);
        const bool pair = present && inside;
        const double xp = inside ? x : 0.0;                    // (x is 0 where it is missing: xp is x' of a pair, else 0)
        const double one = pair ? 1.0 : 0.0;
        cnt[g] += pair ? 1 : 0;
        sx[g] += xp;
        sxx[g] = fma(xp, xp, sxx[g]);
        const double* yrow = Y + (int64_t)sc * Q;
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          const double y = yrow[j];                            // (a scalar register; one * y is y or 0 exactly)
          const double yp = one * y;
          sy[g][j] += yp;
          syy[g][j] = fma(yp, y, syy[g][j]);
          sxy[g][j] = fma(xp, y, sxy[g][j]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g0 + g < n_lags) {
      pairs[(int64_t)(g0 + g) * N + n] = cnt[g];
      double* m = mom + (int64_t)(g0 + g) * M * N + n;
      m[0] = sx[g];
      m[N] = sxx[g];
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        m[(int64_t)(2 + 3 * j) * N] = sy[g][j];
        m[(int64_t)(3 + 3 * j) * N] = syy[g][j];
        m[(int64_t)(4 + 3 * j) * N] = sxy[g][j];
      }
    }
  }
}

// 4. The finish: from the moments r, slope, dof and p of every entry (lag, column, index series), in the final (L, N, q) layout.
// Cxx = Sxx - Sx^2 / n, Cyy = Syy - Sy^2 / n, Cxy = Sxy - Sx Sy / n.  An entry is live when n >= min_pairs, Cxx > 2^-40 Sxx and
// Cyy > 2^-40 Syy (n = 0 makes them NaN, which no comparison passes); a dead entry is NaN with dof 0.  r = Cxy / sqrt(Cxx Cyy),
// clamped by comparisons that pass NaN, and slope = Cxy / Cyy are rounded once to TR.  dof = n, or (rho_x != nullptr, Bretherton et
// al. 1999) min(n, floor(n f)) with rho = rho_x[n] rho_y[j], f = 1 where rho <= 0, else (1 - rho) / (1 + rho).
// p = pearson_two_sided_p(rounded r, dof / 2 - 1, log_norm[dof]), NaN where dof < 3; log_norm is the host's table at 3 .. T.
// Bounds: pairs at i < L N; mom at (l, k < 2 + 3 q, n); rho_x at n < N; rho_y at j < q; log_norm at 3 <= dof <= n <= T; the outputs
// at i < L N q.
template <typename TR>
__global__ void lead_lag_finish_kernel(const int* __restrict__ pairs, const double* __restrict__ mom, int64_t N, int q, int n_lags,
                                       int min_pairs, const double* __restrict__ rho_x, const double* __restrict__ rho_y,
                                       const double* __restrict__ log_norm, TR* __restrict__ r_out, TR* __restrict__ slope_out,
                                       double* __restrict__ p_out, int* __restrict__ dof_out) {
  const int64_t total = (int64_t)n_lags * N * q;
  const int M = ll_moments(q);
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ln = i / q;
    const int j = (int)(i - ln * q);
    const int64_t l = ln / N, n = ln - l * N;
    const int cnt = pairs[ln];
    const double* m = mom + l * M * N + n;
    const double dn = (double)cnt;
    const double sx = m[0], sxx = m[N], sy = m[(int64_t)(2 + 3 * j) * N], syy = m[(int64_t)(3 + 3 * j) * N], sxy = m[(int64_t)(4 + 3 * j) * N];
    const double cxx = sxx - sx * sx / dn, cyy = syy - sy * sy / dn, cxy = sxy - sx * sy / dn;
    const bool live = cnt >= min_pairs && cxx > LL_LIVE * sxx && cyy > LL_LIVE * syy;
    if (!live) {
      r_out[i] = (TR)nan;
      slope_out[i] = (TR)nan;
      p_out[i] = nan;
      dof_out[i] = 0;
      continue;
    }
    double r = cxy / sqrt(cxx * cyy);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    const TR rr = (TR)r;
    int dof = cnt;
    if (rho_x) {
      const double rho = rho_x[n] * rho_y[j];
      const double f = rho <= 0.0 ? 1.0 : (1.0 - rho) / (1.0 + rho);
      const int fl = (int)floor(dn * f);
      dof = fl < cnt ? fl : cnt;
    }
    r_out[i] = rr;
    slope_out[i] = (TR)(cxy / cyy);
    dof_out[i] = dof;
    p_out[i] = dof >= 3 ? pearson_two_sided_p((double)rr, 0.5 * (double)dof - 1.0, log_norm[dof]) : nan;
  }
}

// The launches on stream `st`.  q in [1, LL_MAX_Q]: every q has its own instantiation, with the group ll_group(q).
template <typename TI, int Q>
static inline void lead_lag_moments_q(hipStream_t st, const TI* X, int T, int64_t N, const double* cn, const double* Y, const int* lags,
                                      int n_lags, int* pairs, double* mom) {
  constexpr int G = ll_group(Q);
  const dim3 grid((unsigned)ceil_div(N, LL_COLS), (unsigned)ceil_div(n_lags, G));
  hipLaunchKernelGGL((lead_lag_moments_kernel<TI, Q, G>), grid, dim3(LL_COLS), 0, st, X, T, N, cn, Y, lags, n_lags, pairs, mom);
}

template <typename TI>
static inline void lead_lag_moments(hipStream_t st, const TI* X, int T, int64_t N, const double* cn, const double* Y, int q, const int* lags,
                                    int n_lags, int* pairs, double* mom) {
  switch (q) {
    case 1: lead_lag_moments_q<TI, 1>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 2: lead_lag_moments_q<TI, 2>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 3: lead_lag_moments_q<TI, 3>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 4: lead_lag_moments_q<TI, 4>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 5: lead_lag_moments_q<TI, 5>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 6: lead_lag_moments_q<TI, 6>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 7: lead_lag_moments_q<TI, 7>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    case 8: lead_lag_moments_q<TI, 8>(st, X, T, N, cn, Y, lags, n_lags, pairs, mom); break;
    default: throw Error(XMCA_ERR_INVALID, "lead_lag_maps: between 1 and 8 index series are supported");
  }
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
