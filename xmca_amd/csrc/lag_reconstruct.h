// Reconstructed components of extended EOFs.  With Z_sel the q selected eigenvectors of the centred lag-summed Gram
// matrix (q x T'), X_j = X[j tau : j tau + T', :] and P the (M q) x N stack of the products Z_sel X_j, the reconstruction is
//   R = diag(1 / c) A~ P,    A~[t][j q + c] = Z_sel[c][t - j tau] where 0 <= t - j tau < T', else 0     (T x M q),
// c_t the number of windows that hold time step t: the diagonal averaging of the truncated embedded matrix as one product.  The
// window means the centring took out come back through M more columns of A~ (the indicators [0 <= t - j tau < T']) against M more
// rows of P (the means of the M windows of every column of the field).  The kernels here form A~, 1 / c and the window means.
// Float64 results, memory-bound, no atomics: every sum has a fixed order, so a call repeats its bits.
#pragma once
#include <algorithm>
#include <vector>
#include "kernels.h"

namespace xmca {

constexpr int LAG_MEAN_CHUNKS = 32;              // a segment of the window means is cut into pieces of ceil(T / LAG_MEAN_CHUNKS) rows

// Zsel[c][:] = Z[sel[c]][:], rows of T' values
__global__ void lag_select_rows_kernel(const double* __restrict__ Z, int Tp, const int* __restrict__ sel, int q, double* __restrict__ Zsel) {
  const int64_t total = (int64_t)q * Tp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / Tp, s = i - c * Tp;
    Zsel[i] = Z[(int64_t)sel[c] * Tp + s];
  }
}

// A~ (T x kin, dense, kin = M (q + with_ind), T = T' + (M - 1) tau) and inv_count[t] = 1 / c_t from Z (q x T', row c the vector of
// column c).  Pure placement, consecutive lanes along the columns of a row; every element is written, the zeros too.  The caller
// has checked tau <= T' or M == 1, so that c_t >= 1.
__global__ void lag_expand_kernel(const double* __restrict__ Z, int q, int Tp, int M, int tau, int with_ind, double* __restrict__ A,
                                  double* __restrict__ inv_count) {
  const int T = Tp + (M - 1) * tau, mq = M * q, kin = mq + (with_ind ? M : 0);
  const int64_t total = (int64_t)T * kin;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = first; i < total; i += step) {
    const int t = (int)(i / kin), col = (int)(i - (int64_t)t * kin);
    double v;
    if (col < mq) {
      const int j = col / q, c = col - j * q;
      const int64_t s = (int64_t)t - (int64_t)j * tau;
      v = (s >= 0 && s < Tp) ? Z[(int64_t)c * Tp + s] : 0.0;
    } else {
      const int64_t s = (int64_t)t - (int64_t)(col - mq) * tau;
      v = (s >= 0 && s < Tp) ? 1.0 : 0.0;
    }
    A[i] = v;
  }
  for (int64_t t = first; t < T; t += step) {
    int count = 0;
    for (int j = 0; j < M; ++j) {
      const int64_t s = t - (int64_t)j * tau;
      count += (s >= 0 && s < Tp) ? 1 : 0;
    }
    inv_count[t] = 1.0 / (double)count;
  }
}

static inline void lag_expand(hipStream_t st, const double* Z, int q, int Tp, int M, int tau, bool with_ind, double* A, double* inv_count) {
  const int64_t T = (int64_t)Tp + (int64_t)(M - 1) * tau, kin = (int64_t)M * (q + (with_ind ? 1 : 0));
  XMCA_CHECK(q >= 1 && Tp >= 1 && M >= 1 && tau >= 1 && (M == 1 || tau <= Tp) && T <= INT32_MAX && kin <= INT32_MAX, XMCA_ERR_INVALID,
             "lag_expand: the embedding leaves time steps outside every window, or is too large");
  hipLaunchKernelGGL(lag_expand_kernel, ew_grid(T * kin), dim3(EW_BLOCK), 0, st, Z, q, Tp, M, tau, with_ind ? 1 : 0, A, inv_count);
  XMCA_HIP(hipGetLastError());
}

// The window means in one pass over the field.  The rows are cut at the sorted boundaries {j tau} u {j tau + T'}: a window is a run
// of whole segments.  A segment is cut again into pieces of at most ceil(T / LAG_MEAN_CHUNKS) rows, so the cut depends on the shape
// alone.  The table the two kernels read (ints): first row of every piece, n_pieces end rows, the first piece of every segment and
// n_pieces at the end (n_seg + 1), the first and one-past-last segment of every window (2 M).
struct LagMeanPlan {
  int n_pieces = 0, n_seg = 0;
  std::vector<int> table;
};

static inline LagMeanPlan lag_mean_plan(int T, int M, int tau) {
  const int Tp = T - (M - 1) * tau;
  std::vector<int> bounds;
  for (int j = 0; j < M; ++j) { bounds.push_back(j * tau); bounds.push_back(j * tau + Tp); }
  std::sort(bounds.begin(), bounds.end());
  bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());
  LagMeanPlan plan;
  plan.n_seg = (int)bounds.size() - 1;
  const int len = std::max(1, ceil_div(T, LAG_MEAN_CHUNKS));
  std::vector<int> r0, r1, seg_first;
  for (int s = 0; s < plan.n_seg; ++s) {
    seg_first.push_back((int)r0.size());
    for (int r = bounds[(size_t)s]; r < bounds[(size_t)s + 1]; r += len) { r0.push_back(r); r1.push_back(std::min(r + len, bounds[(size_t)s + 1])); }
  }
  plan.n_pieces = (int)r0.size();
  seg_first.push_back(plan.n_pieces);
  plan.table = r0;
  plan.table.insert(plan.table.end(), r1.begin(), r1.end());
  plan.table.insert(plan.table.end(), seg_first.begin(), seg_first.end());
  for (int j = 0; j < M; ++j) {
    const int a = (int)(std::lower_bound(bounds.begin(), bounds.end(), j * tau) - bounds.begin());
    const int b = (int)(std::lower_bound(bounds.begin(), bounds.end(), j * tau + Tp) - bounds.begin());
    plan.table.push_back(a);
    plan.table.push_back(b);
  }
  return plan;
}

// part[p][n] = sum of the rows of piece p = blockIdx.y of column n, rows in increasing order, in float64 whatever the field's type.
// Lanes along the columns: a row of a workgroup is 256 consecutive elements.
template <typename TI>
__global__ __launch_bounds__(256) void lag_window_mean_kernel(const TI* __restrict__ X, int64_t N, const int* __restrict__ table,
                                                              int n_pieces, double* __restrict__ part) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int p = blockIdx.y;
  const int r0 = table[p], r1 = table[n_pieces + p];
  const TI* x = X + (int64_t)r0 * N + n;
  double acc = 0.0;
#pragma unroll 4
  for (int r = r0; r < r1; ++r, x += N) acc += (double)*x;
  part[(int64_t)p * N + n] = acc;
}

// means[j][n] = (the segments of window j = blockIdx.y added in increasing order, a segment its pieces in increasing order) / T'
__global__ __launch_bounds__(256) void lag_window_mean_finish_kernel(const double* __restrict__ part, int64_t N, const int* __restrict__ table,
                                                                     int n_pieces, int n_seg, int Tp, double* __restrict__ means) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int j = blockIdx.y;
  const int* seg_first = table + 2 * n_pieces;
  const int* win = seg_first + n_seg + 1;
  double acc = 0.0;
  for (int s = win[2 * j]; s < win[2 * j + 1]; ++s) {
    double seg = part[(int64_t)seg_first[s] * N + n];
    for (int p = seg_first[s] + 1; p < seg_first[s + 1]; ++p) seg += part[(int64_t)p * N + n];
    acc += seg;
  }
  means[(int64_t)j * N + n] = acc / (double)Tp;
}

// means (M x N, dense, float64) of the T x N field X (dense).  `table` and `part` are the caller's (they must outlive the kernels).
template <typename TI>
static inline void lag_window_means(hipStream_t st, const TI* X, int T, int64_t N, int M, int tau, double* means, DevBuf<int>& table,
                                    DevBuf<double>& part) {
  const int64_t Tp = (int64_t)T - (int64_t)(M - 1) * tau;
  XMCA_CHECK(M >= 1 && tau >= 1 && Tp >= 1 && N >= 1, XMCA_ERR_INVALID, "lag_window_means: the embedding does not fit the field");
  const LagMeanPlan plan = lag_mean_plan(T, M, tau);
  XMCA_CHECK(plan.n_pieces <= 65535 && M <= 65535, XMCA_ERR_UNSUPPORTED, "lag_window_means: too many lags");
  XMCA_HIP(hipMemcpyAsync(table.ensure(plan.table.size()), plan.table.data(), sizeof(int) * plan.table.size(), hipMemcpyHostToDevice, st));
  XMCA_HIP(hipStreamSynchronize(st));          // (the plan is a host temporary)
  part.ensure((size_t)plan.n_pieces * N);
  const unsigned bx = (unsigned)ceil_div(N, (int64_t)256);
  hipLaunchKernelGGL((lag_window_mean_kernel<TI>), dim3(bx, (unsigned)plan.n_pieces), dim3(256), 0, st, X, N, (const int*)table.get(),
                     plan.n_pieces, part.get());
  hipLaunchKernelGGL(lag_window_mean_finish_kernel, dim3(bx, (unsigned)M), dim3(256), 0, st, (const double*)part.get(), N,
                     (const int*)table.get(), plan.n_pieces, plan.n_seg, (int)Tp, means);
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
