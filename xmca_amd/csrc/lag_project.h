// Monte-Carlo SSA test of extended EOFs: the projection of a surrogate field R (T x N) on the data's extended
// EOFs.  With V_j (N x k) the lag-j patterns, W = R [V_0 | ... | V_{M-1}] (T x M k, one thin GEMM over the whole surrogate),
//   Q[t][c] = sum_{j < M} W[t + j tau][j k + c]          (T' x k, T' = T - (M - 1) tau)   = (Y_R v_c)[t],
//   Lambda_c = sum_t (Q[t][c] - mean_t Q[.][c])^2                                          = || H Y_R v_c ||^2.
// The embedded surrogate Y_R is never formed.  The column scale d_c (sample standard deviation of the field's columns) is folded
// into the patterns once, so a surrogate of unit variance is never rescaled.  Everything here is float64 on small planes,
// memory-bound, and free of atomics: every sum has a fixed order, so a call repeats its bits.
#pragma once
#include "kernels.h"

namespace xmca {

constexpr int LAGP_ROWS = 32;                    // rows of Q per workgroup of the projection kernels (xmca_lag_project_tile)
constexpr int LAGP_COLS = 64;                    // ... and its columns (modes)

// ---- column scale -----------------------------------------------------------------------------------------------------------
// Sums of the columns of x (rows x cols) over the chunks of the column pass (column_pass.h): part[chunk][c], lanes along c
template <typename T>
struct LagpColSum {
  const T* x; int64_t cols; double* part;
  __device__ void operator()(const ColChunk& k) const {
    double s = 0.0;
    for (int r = k.r0; r < k.r1; ++r) s += (double)x[(int64_t)r * cols + k.c];
    part[k.at] = s;
  }
};

// Sums of the squared deviations from the column mean over the same chunks: the mean is the sum of `part` over rows, formed
// alike by every chunk; dev[chunk][c]
template <typename T>
struct LagpColDev {
  const T* x; int rows; int64_t cols; const double* part; double* dev;
  __device__ void operator()(const ColChunk& k) const {
    const double m = chunk_sum(part, k.chunks, cols, k.c) / rows;
    double q = 0.0;
    for (int r = k.r0; r < k.r1; ++r) {
      const double d = (double)x[(int64_t)r * cols + k.c] - m;
      q = fma(d, d, q);
    }
    dev[k.at] = q;
  }
};

// d[c] = sqrt(sum of the chunks of dev / (rows - 1)): the sample standard deviation, ddof = 1
struct LagpColScale {
  const double* dev; int chunks, rows; int64_t cols; double* d;
  __device__ void operator()(int64_t c) const { d[c] = sqrt(chunk_sum(dev, chunks, cols, c) / (double)(rows - 1)); }
};

// B[r][n] = P[r][n] |scale[r mod k]| d[n] in the element type of the GEMM's operand: the unit-norm patterns (scale: that of
// eeof_sign_norm_kernel; the sign does not matter to a squared norm) times the column scale (d == nullptr: left out).
// P, B: M k rows of N values.
template <typename TO>
__global__ void lagp_scale_patterns_kernel(const double* __restrict__ P, const double* __restrict__ scale, const double* __restrict__ d,
                                           int k, int64_t N, int64_t total, TO* __restrict__ B) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / N, n = i - r * N;
    double v = P[i] * fabs(scale[r % k]);
    if (d) v *= d[n];
    B[i] = (TO)v;
  }
}

template <typename TI>
void lag_column_scale(hipStream_t st, const TI* x, int rows, int64_t cols, double* d, DevBuf<double>& part, DevBuf<double>& dev) {
  const int chunks = col_chunks(rows);
  part.ensure((size_t)chunks * cols);
  dev.ensure((size_t)chunks * cols);
  column_pass(st, rows, cols, chunks, LagpColSum<TI>{x, cols, part.get()});
  column_pass(st, rows, cols, chunks, LagpColDev<TI>{x, rows, cols, part.get(), dev.get()});
  column_finish(st, cols, LagpColScale{dev.get(), chunks, rows, cols, d});
  XMCA_HIP(hipGetLastError());
}

// ---- projection -------------------------------------------------------------------------------------------------------------
// One tile of LAGP_ROWS rows x LAGP_COLS columns of Q per workgroup.  W: T rows of ldw = M k values; every read of a valid output
// lies inside it: t + j tau <= T' - 1 + (M - 1) tau = T - 1 and j k + c < M k.  The lanes run along the columns of a row first, so
// a wave reads whole runs of a row of W; the M terms are added in the order j = 0 .. M-1.  Q[t][c] goes to global memory and
// part[tile][c] = the sum of the tile's rows of column c, first row first.
__global__ __launch_bounds__(256) void lagp_shift_sum_kernel(const double* __restrict__ W, int64_t ldw, int np, int M, int tau, int k,
                                                             double* __restrict__ Q, double* __restrict__ part) {
  __shared__ double tile[LAGP_ROWS * LAGP_COLS];
  const int t0 = (int)blockIdx.x * LAGP_ROWS, c0 = (int)blockIdx.y * LAGP_COLS;
  const int kc = min(LAGP_COLS, k - c0), rows = min(LAGP_ROWS, np - t0);
  for (int i = threadIdx.x; i < rows * kc; i += 256) {
    const int r = i / kc, cl = i - r * kc;
    const double* w = W + (int64_t)(t0 + r) * ldw + (c0 + cl);
    double acc = w[0];
    for (int j = 1; j < M; ++j) acc += w[(int64_t)j * ((int64_t)tau * ldw + k)];
    Q[(int64_t)(t0 + r) * k + (c0 + cl)] = acc;
    tile[r * LAGP_COLS + cl] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < kc) {
    double s = tile[threadIdx.x];
    for (int r = 1; r < rows; ++r) s += tile[r * LAGP_COLS + threadIdx.x];
    part[(int64_t)blockIdx.x * k + (c0 + (int)threadIdx.x)] = s;
  }
}

// The same tiles: the mean of column c is the sum of part[.][c] (tile 0 first) over T', formed alike by every workgroup;
// sq[tile][c] = the sum of (Q[t][c] - mean)^2 over the tile's rows, first row first
__global__ __launch_bounds__(256) void lagp_center_square_kernel(const double* __restrict__ Q, const double* __restrict__ part, int np, int k,
                                                                 double* __restrict__ sq) {
  __shared__ double tile[LAGP_ROWS * LAGP_COLS];
  __shared__ double mean[LAGP_COLS];
  const int t0 = (int)blockIdx.x * LAGP_ROWS, c0 = (int)blockIdx.y * LAGP_COLS;
  const int kc = min(LAGP_COLS, k - c0), rows = min(LAGP_ROWS, np - t0);
  if ((int)threadIdx.x < kc) {
    double s = 0.0;
#pragma unroll 8          // (the loads of a batch are issued together; the adds keep their order)
    for (int b = 0; b < (int)gridDim.x; ++b) s += part[(int64_t)b * k + (c0 + (int)threadIdx.x)];
    mean[threadIdx.x] = s / (double)np;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rows * kc; i += 256) {
    const int r = i / kc, cl = i - r * kc;
    const double d = Q[(int64_t)(t0 + r) * k + (c0 + cl)] - mean[cl];
    tile[r * LAGP_COLS + cl] = d * d;
  }
  __syncthreads();
  if ((int)threadIdx.x < kc) {
    double s = tile[threadIdx.x];
    for (int r = 1; r < rows; ++r) s += tile[r * LAGP_COLS + threadIdx.x];
    sq[(int64_t)blockIdx.x * k + (c0 + (int)threadIdx.x)] = s;
  }
}

// out[c] = the sum of sq[.][c], tile 0 first
__global__ void lagp_finish_kernel(const double* __restrict__ sq, int tiles, int k, double* __restrict__ out) {
  const int c = (int)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < tiles; ++b) s += sq[(int64_t)b * k + c];
  out[c] = s;
}

// Lambda (k values at `out`) from W (T x M k, dense).  Q (T' k values) and part (2 tiles k) are the caller's: they must outlive
// the kernels on `st`.
static inline void lag_project(hipStream_t st, const double* W, int T, int M, int tau, int k, double* Q, double* part, double* out) {
  const int np = T - (M - 1) * tau;
  XMCA_CHECK(M >= 1 && tau >= 1 && k >= 1 && np >= 1, XMCA_ERR_INVALID, "lag_project: the embedding does not fit the matrix");
  const int tiles = ceil_div(np, LAGP_ROWS);
  const dim3 grid((unsigned)tiles, (unsigned)ceil_div(k, LAGP_COLS));
  double* sq = part + (size_t)tiles * k;
  hipLaunchKernelGGL(lagp_shift_sum_kernel, grid, dim3(256), 0, st, W, (int64_t)M * k, np, M, tau, k, Q, part);
  hipLaunchKernelGGL(lagp_center_square_kernel, grid, dim3(256), 0, st, (const double*)Q, (const double*)part, np, k, sq);
  hipLaunchKernelGGL(lagp_finish_kernel, dim3((unsigned)ceil_div(k, 256)), dim3(256), 0, st, (const double*)sq, tiles, k, out);
  XMCA_HIP(hipGetLastError());
}
static inline size_t lag_project_scratch(int np, int k) { return (size_t)2 * ceil_div(np, LAGP_ROWS) * k; }

}  // namespace xmca
