// Time filter: a direct FIR filter along time of a T x N field with missing values (NaN), xmca_amd.prepare.time_filter.
// With L = 2 h + 1 weights w the smoother is the correlation S[t][n] = sum_{k < L} w[k] x[t + k - h][n], one float64 fma chain in
// ascending k that starts from +0.0; the output is S or x - S, rounded once to the field's type.  Strict: NaN where any entry of the
// window is missing or outside the record.  Renormalise: S = num / den, the chains of w x and of w over the present entries of
// the window (steps outside the record count as missing); NaN where x[t][n] itself is missing or den < den_min.  One kernel reads
// the field in its own type and writes the result: no mask plane, no widened plane, no atomic, no scratch - a call repeats its
// bits.
#pragma once
#include <limits>

#include "kernels.h"

namespace xmca {

constexpr int TF_COLS = 256;                     // columns of a tile: one lane each (xmca_time_filter_tile)
constexpr int TF_ROWS = 16;                      // output rows of a tile: a lane's accumulators, held in registers (32 measured slower)
constexpr int TF_MAX_WEIGHTS = 1025;             // most weights: they sit in LDS between TF_ROWS - 1 zeros and the zeros of the last piece
constexpr int TF_LDS = TF_MAX_WEIGHTS + 3 * TF_ROWS;
static_assert(TF_ROWS >= 1 && TF_ROWS <= 32, "a lane marks the rows of its tile that hold a NaN in one 32-bit word");
static_assert(TF_MAX_WEIGHTS % 2 == 1, "a filter has a centre");

// The rows r of a tile whose window holds row j of the tile's input span (j = 0 is the first row of the halo): 0 <= j - r < L
__device__ static inline unsigned tf_rows_of(int j, int L) {
  const int lo = j - L + 1 > 0 ? j - L + 1 : 0;
  const int hi = j < TF_ROWS - 1 ? j : TF_ROWS - 1;
  return lo > hi ? 0u : (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo);
}

// The filter.  A workgroup owns TF_ROWS output rows x TF_COLS columns; a lane owns one column n and keeps the TF_ROWS accumulators
// of its tile (and, RENORM, as many denominators) in registers.  The weights are staged once in LDS as wp[p] = w[p - (TF_ROWS - 1)],
// zeros on both sides, and read back as broadcasts.  The lane streams the TF_ROWS + L - 1 input rows of the tile - its rows and
// the 2 h halo rows, each loaded once - in pieces of TF_ROWS rows: row i of piece b is row j = TF_ROWS b + i of the span, it meets
// output row r with the weight k = j - r = wp[TF_ROWS b + (i - r + TF_ROWS - 1)], an LDS address that is the piece's base plus a
// constant, and where k lies outside [0, L) the staged weight is zero.  For one output row the pieces and their rows ascend, so
// the chain runs k = 0 .. L - 1.  A missing entry enters the chains as x = 0 (RENORM: with presence 0, so num and den skip it) and,
// strict, sets the bits tf_rows_of(j) of the lane's NaN word; so does a row outside the record, which is never loaded.
// t_first: the first output row (h for edges = 'trim', else 0); n_out: the number of output rows; out row o is time step t_first + o.
// Bounds: X is read at rows [max(0, t0 - h), min(T, t0 + TF_ROWS + h)) and - COMPLEMENT or RENORM - again at the tile's own rows
// below T, columns n < N; out is written at rows o < n_out, columns n < N; wp at p < TF_ROWS (n_pieces + 1) <= TF_LDS.
template <typename TI, bool RENORM, bool COMPLEMENT>
__global__ __launch_bounds__(TF_COLS) void time_filter_kernel(const TI* __restrict__ X, int T, int64_t N, const double* __restrict__ w, int L,
                                                              double den_min, int t_first, int n_out, TI* __restrict__ out) {
  constexpr int R = TF_ROWS;
  __shared__ double wp[TF_LDS];
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * TF_COLS + tid;
  const bool live = n < N;
  const int h = L / 2;
  const int o0 = (int)blockIdx.y * R;               // first output row of the tile
  const int t0 = t_first + o0;                      // its time step
  const int rows = n_out - o0 < R ? n_out - o0 : R;
  const TI nan = std::numeric_limits<TI>::quiet_NaN();
  if (!RENORM && (t0 + rows - 1 < h || t0 > T - 1 - h)) {          // no window of the tile lies inside the record (the whole workgroup)
    if (live)
      for (int r = 0; r < rows; ++r) out[(int64_t)(o0 + r) * N + n] = nan;
    return;
  }
  const int span = R + L - 1;                       // input rows of the tile, row j at time step t0 - h + j
  const int n_pieces = (span + R - 1) / R;
  for (int p = tid; p < R * (n_pieces + 1); p += TF_COLS) {
    const int k = p - (R - 1);
    wp[p] = (k >= 0 && k < L) ? w[k] : 0.0;
  }
  __syncthreads();
  if (!live) return;
  double num[R], den[RENORM ? R : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) num[r] = 0.0;
#pragma unroll
  for (int r = 0; r < (RENORM ? R : 1); ++r) den[r] = 0.0;
  unsigned bad = 0u;
  const TI* col = X + n;
  for (int b = 0; b < n_pieces; ++b) {
    double x[R], pr[RENORM ? R : 1];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = b * R + i;
      const int s = t0 - h + j;
      const bool inside = j < span && s >= 0 && s < T;
      // (no branch around the load: a row outside the record or past the span is not read, the load goes to the nearest row of
      // the tile's span inside the record - rows the tile reads anyway)
      const int last = t0 - h + span - 1 < T - 1 ? t0 - h + span - 1 : T - 1;
      const int sc = s < 0 ? 0 : (s < last ? s : last);
      const double v = (double)col[(int64_t)sc * N];
      const bool present = inside && v == v;
      x[i] = present ? v : 0.0;
      if (RENORM)
        pr[i] = present ? 1.0 : 0.0;
      else
        bad |= present ? 0u : tf_rows_of(j, L);
    }
    const double* wb = wp + b * R + (R - 1);
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double wk = wb[i - r];
        num[r] = fma(wk, x[i], num[r]);
        if (RENORM) den[r] = fma(wk, pr[i], den[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < rows) {
      const int t = t0 + r;
      double y = RENORM ? num[r] / den[r] : num[r];
      bool is_nan = RENORM ? den[r] < den_min : ((bad >> r) & 1u) != 0u;
      if (RENORM || COMPLEMENT) {
        const double xc = (double)col[(int64_t)t * N];
        if (RENORM) is_nan = is_nan || xc != xc;
        if (COMPLEMENT) y = xc - y;
      }
      out[(int64_t)(o0 + r) * N + n] = is_nan ? nan : (TI)y;
    }
  }
}

// The filter of the contiguous T x N plane X on stream `st`: w the L weights on the device; out n_out x N with
// n_out = trim ? T - 2 h : T.  The caller has checked L (odd, <= TF_MAX_WEIGHTS), T >= L for trim and the grid's row limit.
template <typename TI>
static inline void time_filter(hipStream_t st, const TI* X, int T, int64_t N, const double* w, int L, bool complement, bool renormalise,
                               double den_min, bool trim, TI* out) {
  const int h = L / 2;
  const int t_first = trim ? h : 0;
  const int n_out = trim ? T - 2 * h : T;
  const dim3 grid((unsigned)ceil_div(N, TF_COLS), (unsigned)ceil_div(n_out, TF_ROWS));
  const dim3 block(TF_COLS);
  if (renormalise) {
    if (complement)
      hipLaunchKernelGGL((time_filter_kernel<TI, true, true>), grid, block, 0, st, X, T, N, w, L, den_min, t_first, n_out, out);
    else
      hipLaunchKernelGGL((time_filter_kernel<TI, true, false>), grid, block, 0, st, X, T, N, w, L, den_min, t_first, n_out, out);
  } else {
    if (complement)
      hipLaunchKernelGGL((time_filter_kernel<TI, false, true>), grid, block, 0, st, X, T, N, w, L, den_min, t_first, n_out, out);
    else
      hipLaunchKernelGGL((time_filter_kernel<TI, false, false>), grid, block, 0, st, X, T, N, w, L, den_min, t_first, n_out, out);
  }
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
