// Column regression: every column of a T x N field with missing values (NaN) is fitted by least squares on the
// k <= REG_K columns of a T x k basis B over its present entries, and the residual x - B c replaces the field - the seasonal
// cycle and trend removed, xmca_amd.prepare.anomalies.  Per column the normal equations (sum_present b b^T) c = sum_present b x
// are formed by two thin products of the library's GEMM (the basis rows against the zero-filled plane, their pair products
// against the presence plane); the kernels here are the passes around them: the mask / widen pass, the packed Cholesky solve
// with one lane per column, and the residual pass in the form of gap_fill_kernel.  Everything is float64 in an order fixed by
// the shape and nothing uses an atomic, so a call repeats its bits.  Mask bytes as in gap_fill.h: 0 present, 1 missing.
#pragma once
#include <limits>

#include "kernels.h"

namespace xmca {

constexpr int REG_K = 16;                        // most basis columns: a lane holds that many coefficients in registers
constexpr int REG_COLS = 256;                    // columns of a residual tile: one lane each (xmca_reg_residual_tile)
constexpr int REG_ROWS = 64;                     // rows of a residual tile: their basis rows are staged through LDS at once
constexpr int REG_SOLVE_LANES = 64;              // columns per workgroup of the solve kernel: one wave
constexpr double REG_PIVOT_MIN = 1e-8;           // a Cholesky pivot must exceed this times its diagonal entry (the definition)
static_assert((REG_ROWS * REG_K) % REG_COLS == 0, "the lanes stage the basis rows of a tile in whole rounds");

static inline int reg_packed(int k) { return k * (k + 1) / 2; }      // entries of the packed lower triangle, (i, j <= i) at i (i + 1) / 2 + j

// The mask / widen pass over the T x N plane X: mask = 0 and wide = (double)x where x is present, mask = 1 and wide = 0 where it
// is NaN; pres (nullable) the presence plane 1 / 0 in float64 (the operand of the normal-matrix product); part[block] = the
// block's number of missing entries (lanes strided, then the block's tree: integers in float64, exact below 2^53).
template <typename TI>
__global__ __launch_bounds__(EW_BLOCK) void reg_mask_kernel(const TI* __restrict__ X, int64_t total, unsigned char* __restrict__ mask,
                                                            double* __restrict__ wide, double* __restrict__ pres, double* __restrict__ part) {
  __shared__ double red[4];
  double missing = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * EW_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_BLOCK) {
    const double v = (double)X[i];
    const bool present = v == v;
    mask[i] = present ? 0 : 1;
    wide[i] = present ? v : 0.0;
    if (pres) pres[i] = present ? 1.0 : 0.0;
    missing += present ? 0.0 : 1.0;
  }
  missing = block_sum_256(missing, red);
  if (threadIdx.x == 0) part[blockIdx.x] = missing;
}

// out[0] = the sum of the n_part partials: one workgroup, lanes strided, then the block's tree
__global__ __launch_bounds__(256) void reg_count_kernel(const double* __restrict__ part, int n_part, double* __restrict__ out) {
  __shared__ double red[4];
  double tot = 0.0;
  for (int i = threadIdx.x; i < n_part; i += 256) tot += part[i];
  tot = block_sum_256(tot, red);
  if (threadIdx.x == 0) out[0] = tot;
}

// The solve: one lane per column n, K basis columns (a template parameter: the packed matrix and the right-hand side stay in
// registers, every loop is unrolled and every index a constant).  nm holds the packed normal matrix and, behind it, the number
// of present entries: value e of column n at nm[e * es + n * ns] - (es, ns) = (N, 1) for a matrix per column, (1, 0) for one
// matrix shared by all columns (no entry of the field is missing).  rhs is K x N.  Cholesky A = L L^T in the order of the basis
// columns; the pivot of step j is d_j = A[j][j] - sum_{i < j} L[j][i]^2, and the column is fitted when it has at least K present
// entries and every d_j > REG_PIVOT_MIN * A[j][j] (a comparison that a NaN or a zero diagonal entry fails).  A fitted column gets
// its K coefficients (forward and back substitution) and the byte 1; any other column NaN coefficients and the byte 0.
template <int K>
__global__ __launch_bounds__(REG_SOLVE_LANES) void reg_solve_kernel(const double* __restrict__ nm, int64_t es, int64_t ns,
                                                                    const double* __restrict__ rhs, int64_t N, double* __restrict__ coef,
                                                                    unsigned char* __restrict__ fitted) {
  constexpr int M = K * (K + 1) / 2;
  const int64_t n = (int64_t)blockIdx.x * REG_SOLVE_LANES + threadIdx.x;
  if (n >= N) return;
  double a[M], y[K];
#pragma unroll
  for (int e = 0; e < M; ++e) a[e] = nm[(int64_t)e * es + n * ns];
#pragma unroll
  for (int c = 0; c < K; ++c) y[c] = rhs[(int64_t)c * N + n];
  bool ok = nm[(int64_t)M * es + n * ns] >= (double)K;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double diag = a[j * (j + 1) / 2 + j];
    double d = diag;
#pragma unroll
    for (int i = 0; i < j; ++i) d = fma(-a[j * (j + 1) / 2 + i], a[j * (j + 1) / 2 + i], d);
    ok = ok && d > REG_PIVOT_MIN * diag;
    const double l = sqrt(d);
    a[j * (j + 1) / 2 + j] = l;
#pragma unroll
    for (int r = j + 1; r < K; ++r) {
      double s = a[r * (r + 1) / 2 + j];
#pragma unroll
      for (int i = 0; i < j; ++i) s = fma(-a[r * (r + 1) / 2 + i], a[j * (j + 1) / 2 + i], s);
      a[r * (r + 1) / 2 + j] = s / l;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {          // L z = y
    double s = y[j];
#pragma unroll
    for (int i = 0; i < j; ++i) s = fma(-a[j * (j + 1) / 2 + i], y[i], s);
    y[j] = s / a[j * (j + 1) / 2 + j];
  }
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {     // L^T c = z
    double s = y[j];
#pragma unroll
    for (int i = j + 1; i < K; ++i) s = fma(-a[i * (i + 1) / 2 + j], y[i], s);
    y[j] = s / a[j * (j + 1) / 2 + j];
  }
#pragma unroll
  for (int c = 0; c < K; ++c) coef[(int64_t)c * N + n] = ok ? y[c] : std::numeric_limits<double>::quiet_NaN();
  fitted[n] = ok ? 1 : 0;
}

// The residual pass.  A workgroup owns REG_ROWS rows x REG_COLS columns; a lane owns one column n and keeps its k coefficients in
// registers.  The basis rows of the tile go through LDS, REG_K values a row (columns past k and rows
// past T staged as zeros), and are read back as broadcasts.  Row by row the lane reads its mask byte and its value of the widened
// plane - loads and stores run along n - and writes x - sum_c B[t][c] coef[c], one fma chain c = 0 .. K - 1 in float64 that
// starts from x, rounded once to the output's type; NaN where the mask byte is set or the column is not fitted.  K = k is a
// template parameter: the chain is exactly k long and the coefficients are registers at every k.
// Bounds: mask, wide and out are touched only for t < T and n < N; coef and fitted only for n < N and c < k; B only for t < T, c < k.
template <typename TO, int K>
__global__ __launch_bounds__(REG_COLS) void reg_residual_kernel(const double* __restrict__ wide, const unsigned char* __restrict__ mask,
                                                                const double* __restrict__ B, const double* __restrict__ coef,
                                                                const unsigned char* __restrict__ fitted, int T, int64_t N,
                                                                TO* __restrict__ out) {
  constexpr int k = K;
  __shared__ double bs[REG_ROWS][REG_K];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * REG_COLS + tid;
  const bool live = n < N;
  const int t_begin = (int)blockIdx.y * REG_ROWS;
  const int rows = T - t_begin < REG_ROWS ? T - t_begin : REG_ROWS;
  for (int e = tid; e < REG_ROWS * REG_K; e += REG_COLS) {
    const int r = e / REG_K, c = e % REG_K;
    bs[r][c] = (r < rows && c < k) ? B[(int64_t)(t_begin + r) * k + c] : 0.0;
  }
  double cf[K];
#pragma unroll
  for (int c = 0; c < K; ++c) cf[c] = live ? coef[(int64_t)c * N + n] : 0.0;
  const bool fit = live && fitted[n] != 0;
  __syncthreads();
  if (!live) return;
  const TO nan = std::numeric_limits<TO>::quiet_NaN();
#pragma unroll 4
  for (int r = 0; r < rows; ++r) {
    const int64_t i = (int64_t)(t_begin + r) * N + n;
    const unsigned char m = mask[i];
    double acc = wide[i];
#pragma unroll
    for (int c = 0; c < K; ++c) acc = fma(-bs[r][c], cf[c], acc);
    out[i] = (m || !fit) ? nan : (TO)acc;
  }
}

// Scratch of the mask pass, the caller's (it must outlive the kernels on `st`)
struct RegMaskScratch {
  DevBuf<double> part, count;
};

// The mask / widen pass on stream `st`; the number of missing entries arrives at w.count[0] (the caller copies it when it wants it)
template <typename TI>
static inline void reg_mask(hipStream_t st, const TI* X, int64_t total, unsigned char* mask, double* wide, double* pres, RegMaskScratch& w) {
  const dim3 grid = ew_grid(total, 4);
  hipLaunchKernelGGL((reg_mask_kernel<TI>), grid, dim3(EW_BLOCK), 0, st, X, total, mask, wide, pres, w.part.ensure(grid.x));
  hipLaunchKernelGGL(reg_count_kernel, dim3(1), dim3(256), 0, st, (const double*)w.part.get(), (int)grid.x, w.count.ensure(1));
  XMCA_HIP(hipGetLastError());
}

template <int K>
static inline void reg_solve_k(hipStream_t st, int k, const double* nm, int64_t es, int64_t ns, const double* rhs, int64_t N, double* coef,
                               unsigned char* fitted) {
  if constexpr (K > REG_K) {
    XMCA_CHECK(false, XMCA_ERR_INVALID, "column_regress: k must lie in [1, 16]");
  } else {
    if (k == K)
      hipLaunchKernelGGL((reg_solve_kernel<K>), dim3((unsigned)ceil_div(N, REG_SOLVE_LANES)), dim3(REG_SOLVE_LANES), 0, st, nm, es, ns, rhs, N,
                         coef, fitted);
    else
      reg_solve_k<K + 1>(st, k, nm, es, ns, rhs, N, coef, fitted);
  }
}

// The solve of N columns with k basis columns: nm, es, ns, rhs as reg_solve_kernel; coef k x N, fitted N bytes
static inline void reg_solve(hipStream_t st, int k, const double* nm, int64_t es, int64_t ns, const double* rhs, int64_t N, double* coef,
                             unsigned char* fitted) {
  XMCA_CHECK(k >= 1 && k <= REG_K, XMCA_ERR_INVALID, "column_regress: k must lie in [1, 16]");
  reg_solve_k<1>(st, k, nm, es, ns, rhs, N, coef, fitted);
  XMCA_HIP(hipGetLastError());
}

template <typename TO, int K>
static inline void reg_residual_k(hipStream_t st, const double* wide, const unsigned char* mask, const double* B, const double* coef,
                                  const unsigned char* fitted, int T, int64_t N, int k, TO* out) {
  if constexpr (K > REG_K) {
    XMCA_CHECK(false, XMCA_ERR_INVALID, "column_residual: k must lie in [1, 16]");
  } else {
    if (k == K) {
      const dim3 grid((unsigned)ceil_div(N, REG_COLS), (unsigned)ceil_div(T, REG_ROWS));
      hipLaunchKernelGGL((reg_residual_kernel<TO, K>), grid, dim3(REG_COLS), 0, st, wide, mask, B, coef, fitted, T, N, out);
    } else {
      reg_residual_k<TO, K + 1>(st, wide, mask, B, coef, fitted, T, N, k, out);
    }
  }
}

// The residual pass on the planes of reg_mask: B T x k (row-major), coef k x N, fitted N bytes, out T x N
template <typename TO>
static inline void reg_residual(hipStream_t st, const double* wide, const unsigned char* mask, const double* B, const double* coef,
                                const unsigned char* fitted, int T, int64_t N, int k, TO* out) {
  XMCA_CHECK(k >= 1 && k <= REG_K, XMCA_ERR_INVALID, "column_residual: k must lie in [1, 16]");
  reg_residual_k<TO, 1>(st, wide, mask, B, coef, fitted, T, N, k, out);
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
