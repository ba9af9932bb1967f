// Streaming (HBM-bound) helper kernels: conversions, plane packing, row/column scaling, row
// normalisation, column centering and the Philox surrogate generator.
#pragma once
#include "common.h"
#include "column_pass.h"

namespace xmca {

// 1/sqrt(x) and 1/x for normal positive x, full double precision: hardware seed (5e-8 relative on gfx950,
// scripts/probes/rsq_accuracy.cpp) + two Newton steps (1.4e-16; a third changes nothing)
__device__ __forceinline__ double jac_rsqrt(const double x) {
  double y = __builtin_amdgcn_rsq(x);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double h = 0.5 * x * y;
    y = fma(y, fma(-h, y, 0.5), y);
  }
  return y;
}
__device__ __forceinline__ double jac_rcp(const double x) {
  double y = __builtin_amdgcn_rcp(x);
#pragma unroll
  for (int it = 0; it < 2; ++it) y = fma(y, fma(-x, y, 1.0), y);
  return y;
}

// single precision: the hardware seeds are accurate to 1 ulp
__device__ __forceinline__ float jac_rsqrt(const float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float jac_rcp(const float x) { return __builtin_amdgcn_rcpf(x); }

constexpr int EW_BLOCK = 256;
static inline dim3 ew_grid(int64_t n, int per_thread = 1) {
  int64_t b = (n + (int64_t)EW_BLOCK * per_thread - 1) / ((int64_t)EW_BLOCK * per_thread);
  if (b > 8192) b = 8192;   // grid-stride beyond that
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

template <typename TI, typename TO>
__global__ void convert_kernel(const TI* __restrict__ in, TO* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (TO)in[i];
}

// interleaved complex (re,im,re,im,...) -> two planes
template <typename TI, typename TO>
__global__ void split_complex_kernel(const TI* __restrict__ in, TO* __restrict__ re, TO* __restrict__ im, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    re[i] = (TO)in[2 * i];
    im[i] = (TO)in[2 * i + 1];
  }
}

// rows x cols block of planes (ld) -> dense output: real (im == nullptr) or interleaved complex; optional conj
template <typename TO>
__global__ void pack_rows_kernel(const double* __restrict__ re, const double* __restrict__ im, int64_t ld, int rows, int cols,
                                 TO* __restrict__ out, int conj) {
  const int64_t n = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols, c = i % cols;
    const double vr = re[r * ld + c];
    if (im) {
      const double vi = im[r * ld + c];
      out[2 * i] = (TO)vr;
      out[2 * i + 1] = (TO)(conj ? -vi : vi);
    } else {
      out[i] = (TO)vr;
    }
  }
}

// EOFs in their final layout (xmca_get_eofs): out[n][c] = sum_m V[m][n] W[m][c] for the mode-major vectors V (planes of TV, rows
// ld apart; Vi == nullptr: real) and a small mixing matrix W (m x q planes in float64; Wi == nullptr: real).  One thread per grid
// point n: the reads of a mode are coalesced over n, the q values of a point are written side by side.  The output is complex
// (interleaved) when V or W is.
template <typename TV, typename TO>
__global__ void eof_mix_kernel(const TV* __restrict__ Vr, const TV* __restrict__ Vi, int64_t ld, int64_t N, int m, int q,
                               const double* __restrict__ Wr, const double* __restrict__ Wi, TO* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const bool oc = Vi || Wi;
  for (int c0 = 0; c0 < q; c0 += 8) {
    double ar[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ai[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int mm = 0; mm < m; ++mm) {
      const double vr = (double)Vr[(int64_t)mm * ld + n], vi = Vi ? (double)Vi[(int64_t)mm * ld + n] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u < q ? c0 + u : q - 1;
        const double wr = Wr[mm * q + c], wi = Wi ? Wi[mm * q + c] : 0.0;
        ar[u] += vr * wr - vi * wi;
        ai[u] += vr * wi + vi * wr;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + u;
      if (c < q) {
        if (oc) { out[2 * (n * q + c)] = (TO)ar[u]; out[2 * (n * q + c) + 1] = (TO)ai[u]; }
        else out[n * q + c] = (TO)ar[u];
      }
    }
  }
}
// ... and without a mixing matrix: out[n][c] = V[c][n], a 32 x 32 tile at a time through LDS (both sides coalesced)
template <typename TV, typename TO>
__global__ __launch_bounds__(256) void eof_transpose_kernel(const TV* __restrict__ Vr, const TV* __restrict__ Vi, int64_t ld, int64_t N, int q,
                                                           TO* __restrict__ out) {
  __shared__ double tr[32][33], ti[32][33];
  const int64_t n0 = (int64_t)blockIdx.x * 32;
  const int c0 = (int)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const int64_t n = n0 + tx;
    const bool in = c < q && n < N;
    tr[r][tx] = in ? (double)Vr[(int64_t)c * ld + n] : 0.0;
    ti[r][tx] = (in && Vi) ? (double)Vi[(int64_t)c * ld + n] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t n = n0 + r;
    const int c = c0 + tx;
    if (n < N && c < q) {
      if (Vi) { out[2 * (n * q + c)] = (TO)tr[tx][r]; out[2 * (n * q + c) + 1] = (TO)ti[tx][r]; }
      else out[n * q + c] = (TO)tr[tx][r];
    }
  }
}

// X[r][c] *= s[r] (by_row) or s[c]; both planes
__global__ void scale_kernel(double* __restrict__ re, double* __restrict__ im, int64_t ld, int rows, int cols,
                             const double* __restrict__ s, int by_row, int invert) {
  const int64_t n = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols, c = i % cols;
    double f = s[by_row ? r : c];
    if (invert) f = 1.0 / f;
    re[r * ld + c] *= f;
    if (im) im[r * ld + c] *= f;
  }
}

// G[i][i] += v
__global__ void add_diag_kernel(double* __restrict__ G, int64_t ld, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) G[(int64_t)i * ld + i] += v;
}

// largest |C_ij| / sqrt(C_ii C_jj), i != j, of an n x n Hermitian Gram matrix with a positive diagonal (rows with a zero
// diagonal - null modes - are skipped): how far a set of vectors is from orthogonal.  One row per workgroup (grid-stride);
// row_worst[i] (optional) = the same over j < i only.
__global__ void coherence_kernel(const double* __restrict__ Cr, const double* __restrict__ Ci, int n, int n_check,
                                 unsigned long long* __restrict__ out, double* __restrict__ row_worst) {
  __shared__ double red[4];
  double worst = 0.0;
  for (int i = blockIdx.x; i < n_check; i += gridDim.x) {      // the leading n_check rows / columns of the n x n matrix
    const double dii = Cr[(int64_t)i * n + i];
    double mine = 0.0;                                         // row i against the rows before it (the stronger modes)
    if (dii > 0.0) {
      for (int j = threadIdx.x; j < n_check; j += blockDim.x) {
        const double djj = Cr[(int64_t)j * n + j];
        if (j == i || !(djj > 0.0)) continue;
        const double re = Cr[(int64_t)i * n + j], im = Ci ? Ci[(int64_t)i * n + j] : 0.0;
        double c = sqrt((re * re + im * im) / (dii * djj));
        if (!(c == c)) c = HUGE_VAL;
        worst = fmax(worst, c);
        if (j < i) mine = fmax(mine, c);
      }
    }
    if (row_worst) {
      for (int o = 32; o > 0; o >>= 1) mine = fmax(mine, __shfl_xor(mine, o));
      __syncthreads();
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
      __syncthreads();
      if (threadIdx.x == 0) row_worst[i] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
  if ((threadIdx.x & 63) == 0 && worst > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(worst));
}

// dinv[r] = 1 / Re sum_k A[r][k] conj(B[r][k])   (rows of two r x n plane pairs; 0 when the sum is not positive)
__global__ void row_dot_inverse_kernel(const double* __restrict__ Ar, const double* __restrict__ Ai, const double* __restrict__ Br,
                                       const double* __restrict__ Bi, int n, double* __restrict__ dinv) {
  __shared__ double red[4];
  const int64_t row = (int64_t)blockIdx.x * n;
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    acc += Ar[row + k] * Br[row + k];
    if (Ai) acc += Ai[row + k] * Bi[row + k];
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double d = (red[0] + red[1]) + (red[2] + red[3]);
    dinv[blockIdx.x] = d > 0.0 ? 1.0 / d : 0.0;
  }
}

// out[r] = sum_k A[r][k]   (n x n plane, one row per workgroup)
__global__ void row_sum_kernel(const double* __restrict__ A, int n, double* __restrict__ out) {
  __shared__ double red[4];
  const int64_t row = (int64_t)blockIdx.x * n;
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += blockDim.x) acc += A[row + k];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// exactly Hermitian from nearly Hermitian: (G + G^H) / 2 on the planes of an n x n matrix (imaginary diagonal -> 0)
__global__ void hermitize_kernel(double* __restrict__ Gr, double* __restrict__ Gi, int n) {
  const int64_t total = (int64_t)n * n;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / n), j = (int)(idx % n);
    if (j < i) continue;
    const int64_t a = (int64_t)i * n + j, b = (int64_t)j * n + i;
    const double re = 0.5 * (Gr[a] + Gr[b]);
    Gr[a] = re;
    Gr[b] = re;
    if (Gi) {
      const double im = i == j ? 0.0 : 0.5 * (Gi[a] - Gi[b]);
      Gi[a] = im;
      Gi[b] = -im;
    }
  }
}

// x[i] += v
__global__ void add_const_kernel(double* __restrict__ x, int64_t n, double v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] += v;
}

// Ht[t][s] = col[(t - s) mod T]  (circulant operator from its first column)
template <typename TO>
__global__ void circulant_kernel(const double* __restrict__ col, int T, TO* __restrict__ out) {
  const int64_t n = (int64_t)T * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / T), s = (int)(i % T);
    int d = t - s;
    if (d < 0) d += T;
    out[i] = (TO)col[d];
  }
}

// T x T imaginary operator of the fore/back-cast analytic signal (extend='exp', xmca_amd/_hip.py extended_imag_parts):
// G[t][s] = col3[(t - s) mod 3T] - hbar[s] + sum_k U[t][k] W[s][k] - the middle block of the 3T circulant Hilbert operator, the
// rank-r images of the extensions (U, T x r row-major, already centered) and the row-mean removal of `remove_mean` (hbar: the
// column means of the middle block).  Accumulated in float64, stored in the field's element type.
template <typename TO>
__global__ void extended_operator_kernel(const double* __restrict__ col3, const double* __restrict__ hbar, const double* __restrict__ U,
                                         const double* __restrict__ W, int r, int T, TO* __restrict__ out) {
  const int64_t n = (int64_t)T * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / T), s = (int)(i % T);
    int64_t d = (int64_t)t - s;            // in (-T, T): col3 index d or 3T + d, both < 3T
    if (d < 0) d += 3 * (int64_t)T;
    double g = col3[d] - hbar[s];
    for (int k = 0; k < r; ++k) g += U[(int64_t)t * r + k] * W[(int64_t)s * r + k];
    out[i] = (TO)g;
  }
}

// Orthonormal Fourier vectors of the frequencies kept by the analytic signal: Phi[t][f] = exp(2 pi i f t / T) / sqrt(T),
// f = 0 .. m-1 (m = T/2 + 1 for even T, (T+1)/2 for odd T), and the Hilbert weights h_f of scipy.signal.hilbert
// (1 for DC and Nyquist, 2 otherwise), so that hilbert(x) = Phi diag(h) Phi^H x.
__global__ void fourier_basis_kernel(int T, int m, double* __restrict__ Pr, double* __restrict__ Pi, double* __restrict__ hvec) {
  const int64_t n = (int64_t)T * m;
  const double inv = 1.0 / sqrt((double)T);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / m), f = (int)(i % m);
    const int64_t ft = ((int64_t)f * t) % T;
    double sn, cs;
    sincospi(2.0 * (double)ft / (double)T, &sn, &cs);
    Pr[i] = cs * inv;
    Pi[i] = sn * inv;
    if (i < m) hvec[i] = (i == 0 || (T % 2 == 0 && i == T / 2)) ? 1.0 : 2.0;
  }
}

__global__ void sqrt_clamp_kernel(const double* __restrict__ lam, double* __restrict__ s, int n, double scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) s[i] = sqrt(fmax(lam[i] * scale, 0.0));
}

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// one workgroup per row: row <- conj?(row) / ||row||   (planes, f64).  norms_out (nullable) gets ||row||.
template <typename T>
__global__ __launch_bounds__(256) void normalize_rows_kernel(T* __restrict__ re, T* __restrict__ im, int64_t ld, int cols,
                                                             int conj, double* __restrict__ norms_out) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x;
  double acc = 0.0;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const double a = (double)re[r * ld + c];
    acc += a * a;
    if (im) {
      const double b = (double)im[r * ld + c];
      acc += b * b;
    }
  }
  const double nrm = sqrt(block_sum_256(acc, red));
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  for (int c = threadIdx.x; c < cols; c += 256) {
    re[r * ld + c] = (T)((double)re[r * ld + c] * inv);
    if (im) im[r * ld + c] = (T)((double)im[r * ld + c] * (conj ? -inv : inv));
  }
  if (norms_out && threadIdx.x == 0) norms_out[r] = nrm;
}

// The same for a few LONG rows (the null mode of a centered float32 field with 10^6 grid points: one workgroup walking a
// whole row takes 2.5 ms): a row is cut into chunks of ROWN_CHUNK columns, partial sums of squares per (row, chunk), then
// every chunk scales itself by the sum of its row's partials taken in chunk order (deterministic, no atomics).
constexpr int ROWN_CHUNK = 8192;
template <typename T>
__global__ __launch_bounds__(256) void row_sumsq_chunk_kernel(const T* __restrict__ re, const T* __restrict__ im, int64_t ld, int cols,
                                                              double* __restrict__ part) {
  __shared__ double red[4];
  const int64_t r = blockIdx.y;
  const int c0 = blockIdx.x * ROWN_CHUNK, c1 = min(cols, c0 + ROWN_CHUNK);
  double acc = 0.0;
  for (int c = c0 + threadIdx.x; c < c1; c += 256) {
    const double a = (double)re[r * ld + c];
    acc += a * a;
    if (im) {
      const double b = (double)im[r * ld + c];
      acc += b * b;
    }
  }
  const double s = block_sum_256(acc, red);
  if (threadIdx.x == 0) part[r * gridDim.x + blockIdx.x] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void row_scale_chunk_kernel(T* __restrict__ re, T* __restrict__ im, int64_t ld, int cols, int conj,
                                                              const double* __restrict__ part, double* __restrict__ norms_out) {
  const int64_t r = blockIdx.y;
  double tot = 0.0;
  for (int q = 0; q < (int)gridDim.x; ++q) tot += part[r * gridDim.x + q];
  const double nrm = sqrt(tot);
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  const int c0 = blockIdx.x * ROWN_CHUNK, c1 = min(cols, c0 + ROWN_CHUNK);
  for (int c = c0 + threadIdx.x; c < c1; c += 256) {
    re[r * ld + c] = (T)((double)re[r * ld + c] * inv);
    if (im) im[r * ld + c] = (T)((double)im[r * ld + c] * (conj ? -inv : inv));
  }
  if (norms_out && blockIdx.x == 0 && threadIdx.x == 0) norms_out[r] = nrm;
}
// rows <- conj?(rows) / ||row||: one workgroup per row, or - few long rows - one per chunk of a row
template <typename T>
static inline void normalize_rows(hipStream_t st, T* re, T* im, int64_t ld, int rows, int cols, int conj, double* norms_out,
                                  DevBuf<double>* part_keep = nullptr) {
  // part_keep: where the partial sums of the chunked form live when `st` is not the stream of the calling thread's pool
  if (rows <= 0) return;
  const int chunks = ceil_div(cols, ROWN_CHUNK);
  if (rows >= 256 || chunks < 4) {
    hipLaunchKernelGGL((normalize_rows_kernel<T>), dim3(rows), dim3(256), 0, st, re, im, ld, cols, conj, norms_out);
  } else {
    DevBuf<double> part_here;  // (returned to the stream's pool: the kernels queued here are ahead of its next user)
    DevBuf<double>& part = part_keep ? *part_keep : part_here;
    part.ensure((size_t)rows * chunks);
    hipLaunchKernelGGL((row_sumsq_chunk_kernel<T>), dim3(chunks, rows), dim3(256), 0, st, (const T*)re, (const T*)im, ld, cols, part.get());
    hipLaunchKernelGGL((row_scale_chunk_kernel<T>), dim3(chunks, rows), dim3(256), 0, st, re, im, ld, cols, conj, (const double*)part.get(), norms_out);
  }
  XMCA_HIP(hipGetLastError());
}

// Column passes of the constructor stage: functors of the chunked pass of column_pass.h.
// part_nan[chunk][c] = NaN entries, part_sum[chunk][c] = sum of column c over the rows of the chunk (part_sum may be null)
template <typename T>
struct ColumnPartialSums {
  const T* x; int64_t cols; int* part_nan; double* part_sum;
  __device__ void operator()(const ColChunk& k) const {
    double s = 0.0;
    int nans = 0;
    for (int r = k.r0; r < k.r1; ++r) {
      const double v = (double)x[(int64_t)r * cols + k.c];
      if (v != v) ++nans;
      s += v;
    }
    part_nan[k.at] = nans;
    if (part_sum) part_sum[k.at] = s;
  }
};

// nan_count[c] = sum over chunks; mean[c] = (sum over chunks) / rows   (part_sum and mean may be null)
struct ColumnFinishSums {
  const int* part_nan; const double* part_sum; int chunks, rows; int64_t cols; int* nan_count; double* mean;
  __device__ void operator()(int64_t c) const {
    nan_count[c] = chunk_sum(part_nan, chunks, cols, c);
    if (mean) mean[c] = chunk_sum(part_sum, chunks, cols, c) / rows;
  }
};

// Lag-1 autocorrelation of every column: part[0 / 1 / 2][chunk][c] = sum x, sum x^2 and sum x[t] x[t+1] over
// the rows t of the chunk (the product belongs to the chunk of t: a chunk reads one row past its end);
// ends[0][c] = x[0][c], ends[1][c] = x[rows-1][c].
template <typename T>
struct Lag1Partial {
  const T* x; int rows; int64_t cols; double* part; double* ends;
  __device__ void operator()(const ColChunk& k) const {
    const int64_t c = k.c;
    double s = 0.0, q = 0.0, l = 0.0;
    if (k.r0 < k.r1) {
      double v = (double)x[(int64_t)k.r0 * cols + c];
      if (k.r0 == 0) ends[c] = v;
      for (int r = k.r0; r < k.r1; ++r) {
        const double next = r + 1 < rows ? (double)x[(int64_t)(r + 1) * cols + c] : 0.0;
        s += v;
        q += v * v;
        l += v * next;
        if (r == rows - 1) ends[cols + c] = v;
        v = next;
      }
    }
    const int64_t plane = (int64_t)k.chunks * cols;
    part[k.at] = s;
    part[plane + k.at] = q;
    part[2 * plane + k.at] = l;
  }
};

// phi[c] = sum_t (x[t] - m)(x[t+1] - m) / sum_t (x[t] - m)^2 from the raw sums of the chunks:
// (L - m (2 S - x_0 - x_last) + (rows - 1) m^2) / (Q - rows m^2).  A column that is constant to rounding (the denominator is
// within the rounding error of Q) gives 0: never a NaN.
struct Lag1Finish {
  const double* part; const double* ends; int chunks, rows; int64_t cols; double* phi;
  __device__ void operator()(int64_t c) const {
    const int64_t plane = (int64_t)chunks * cols;
    const double s = chunk_sum(part, chunks, cols, c), q = chunk_sum(part + plane, chunks, cols, c);
    const double l = chunk_sum(part + 2 * plane, chunks, cols, c);
    const double m = s / rows;
    const double den = q - (double)rows * m * m;
    const double num = l - m * (2.0 * s - ends[c] - ends[cols + c]) + (double)(rows - 1) * m * m;
    phi[c] = den > 4.0 * rows * 1.1102230246251565e-16 * q ? num / den : 0.0;
  }
};

// x[r][c] -= mean[c]
template <typename T>
__global__ void subtract_column_means_kernel(T* __restrict__ x, int rows, int64_t cols, const double* __restrict__ mean) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    x[i] = (T)((double)x[i] - mean[i % cols]);
}

// x[r][c] -= mean[c] for the columns without NaN (a column holding one is left as it is); part_sq[chunk][c] = sum of squared deviations over the rows of the chunk
template <typename T>
struct CenterColumnsChunk {
  T* x; int64_t cols; const double* mean; const int* nan_count; double* part_sq;
  __device__ void operator()(const ColChunk& k) const {
    double q = 0.0;
    if (nan_count[k.c] == 0) {
      const double m = mean[k.c];
      for (int r = k.r0; r < k.r1; ++r) {
        const double d = (double)x[(int64_t)r * cols + k.c] - m;
        q += d * d;
        x[(int64_t)r * cols + k.c] = (T)d;
      }
    }
    part_sq[k.at] = q;
  }
};

// stdev[c] = sqrt(sum over chunks / rows)   (columns with NaN: the mean, as before)
struct ColumnFinishStd {
  const double* part_sq; int chunks, rows; int64_t cols; const double* mean; const int* nan_count; double* stdev;
  __device__ void operator()(int64_t c) const {
    const double q = chunk_sum(part_sq, chunks, cols, c);
    stdev[c] = nan_count[c] ? mean[c] : sqrt(q / rows);
  }
};

// out[r][j] = in[r][idx[j]]   (column selection: rows x cols_in -> rows x cols_out)
template <typename T>
__global__ void gather_columns_kernel(const T* __restrict__ in, int64_t cols_in, T* __restrict__ out, int64_t cols_out,
                                      const int64_t* __restrict__ idx, int rows) {
  const int64_t total = (int64_t)rows * cols_out;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols_out, j = i % cols_out;
    out[i] = in[r * cols_in + idx[j]];
  }
}

// x[r][c] = x[r][c] * w[c]  or  x[r][c] / w[c]   (w already in the element type: the host's own operation, bit for bit)
template <typename T>
__global__ void scale_columns_kernel(T* __restrict__ x, int rows, int64_t cols, const T* __restrict__ w, int divide) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const T f = w[i % cols];
    x[i] = divide ? x[i] / f : x[i] * f;
  }
}

// New data of MCA.predict (xmca_predict): out[t][c] = (raw[t][idx[c]] - mean[c]) / std[c] for a rows x n_full row-major block, in
// the element type TI of the data - numpy's `x -= mean; x /= std` bit for bit (a subtraction, then a correctly rounded division:
// nothing to contract) - stored as the product's element type TP.  idx == nullptr: all columns (the contiguous case);
// std == nullptr: no division.  weight (float64, one per kept column) != nullptr: the value is then multiplied by weight[c] in
// double and rounded back to TI - numpy's in-place `x *= w` for a float64 w (a plain multiply for TI = double); the vector is
// re-read per row and stays in L2.  Rows over blockIdx.y, columns over x: no index division per element.
template <typename TI, typename TP>
__global__ void ingest_columns_kernel(const TI* __restrict__ raw, int64_t n_full, const int64_t* __restrict__ idx, int rows,
                                      int64_t cols, const TI* __restrict__ mean, const TI* __restrict__ stdv,
                                      const double* __restrict__ weight, TP* __restrict__ out) {
  for (int t = blockIdx.y; t < rows; t += gridDim.y) {
    const TI* src = raw + (int64_t)t * n_full;
    TP* dst = out + (int64_t)t * cols;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += (int64_t)gridDim.x * blockDim.x) {
      TI v = src[idx ? idx[c] : c];
      v = v - mean[c];
      if (stdv) v = v / stdv[c];
      if (weight) v = (TI)((double)v * weight[c]);
      dst[c] = (TP)v;
    }
  }
}

// Reconstruction epilogue (xmca_reconstruct): one pass from the compact rows x n_keep product C to the final rows x n_full
// float64 layout.  Column j of the output is column col_of[j] of C (col_of == nullptr: j itself), or NaN where col_of[j] < 0;
// kept values become C * std + mean like numpy's `x *= std; x += mean` (two roundings: not contracted), either factor optional.
// inv_weight != nullptr: C / inv_weight[c] first, numpy's `x /= w` (an IEEE division, never a reciprocal multiply).
__global__ void reconstruct_epilogue_kernel(const double* __restrict__ C, int64_t n_keep, const int64_t* __restrict__ col_of, int rows,
                                            int64_t n_full, const double* __restrict__ inv_weight, const double* __restrict__ stdv,
                                            const double* __restrict__ mean, double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int t = blockIdx.y; t < rows; t += gridDim.y) {
    const double* src = C + (int64_t)t * n_keep;
    double* dst = out + (int64_t)t * n_full;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_full; j += (int64_t)gridDim.x * blockDim.x) {
      const int64_t c = col_of ? col_of[j] : j;
      if (c < 0) {
        dst[j] = __builtin_nan("");
        continue;
      }
      double v = src[c];
      if (inv_weight) v = v / inv_weight[c];
      if (stdv) v = v * stdv[c];
      if (mean) v = v + mean[c];
      dst[j] = v;
    }
  }
}

// 2-D grid of the two kernels above: columns in blocks of EW_BLOCK (at most 64 blocks), rows over y (at most 4096 at a time)
static inline dim3 row_col_grid(int64_t rows, int64_t cols) {
  int64_t bx = (cols + EW_BLOCK - 1) / EW_BLOCK;
  if (bx > 64) bx = 64;
  if (bx < 1) bx = 1;
  int64_t by = rows < 4096 ? rows : 4096;
  if (by < 1) by = 1;
  return dim3((unsigned)bx, (unsigned)by);
}

// ------------------------------------------------------------------------------------------------
// Strided device ingest (xmca_set_field_strided, the device entrance of xmca_predict_strided): a T x N view of device memory with
// element (t, n) at src[t * stride_t + n * stride_n] -> a contiguous row-major T x N array.  Pure copies (the bits of every
// element, NaN payloads included), 64-bit index arithmetic throughout, no scratch, no atomics.  Three regimes, chosen on the
// host from the strides (ingest_regime).
// ------------------------------------------------------------------------------------------------
constexpr int INGEST_ROWS = 0, INGEST_TRANSPOSE = 1, INGEST_GATHER = 2;
constexpr int INGEST_TILE = 64;      // edge of the transpose tile: one wave reads / writes 64 consecutive elements

// rows contiguous (stride_n == 1), `pitch` elements apart: a coalesced copy.  A row whose source and destination both start on a
// 16-byte boundary moves 16 bytes per lane and finishes with single elements; any other row (a base aligned to the element
// only, a pitch that moves the alignment from row to row) moves single elements.  The choice is uniform over the workgroup.
template <typename T>
__global__ void ingest_rows_kernel(const T* __restrict__ src, int64_t pitch, int64_t rows, int64_t cols, T* __restrict__ dst) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = blockIdx.y; t < rows; t += gridDim.y) {
    const T* s = src + t * pitch;
    T* d = dst + t * cols;
    int64_t done = 0;
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
      const int64_t nv = cols / V;
      for (int64_t i = i0; i < nv; i += step) reinterpret_cast<vec_t*>(d)[i] = reinterpret_cast<const vec_t*>(s)[i];
      done = nv * V;
    }
    for (int64_t i = done + i0; i < cols; i += step) d[i] = s[i];
  }
}

// time is the fast axis (stride_t == 1), columns `pitch` elements apart: a transpose, one 64 x 64 tile at a time through LDS.  A
// wave reads 64 consecutive time steps of one column and writes 64 consecutive columns of one time step.  The tile rows are
// padded by one element: the row-wise stores and the column-wise loads (65 dwords apart for float, 130 for double - 32 lanes on
// 32 / 64 distinct banks) are both free of bank conflicts.  Partial tiles at both edges are masked.
template <typename T>
__global__ __launch_bounds__(256) void ingest_transpose_kernel(const T* __restrict__ src, int64_t pitch, int64_t rows, int64_t cols,
                                                              T* __restrict__ dst) {
  __shared__ T tile[INGEST_TILE][INGEST_TILE + 1];
  const int tx = threadIdx.x & (INGEST_TILE - 1), ty = threadIdx.x / INGEST_TILE;      // 64 x 4
  const int64_t tiles_t = (rows + INGEST_TILE - 1) / INGEST_TILE, tiles_n = (cols + INGEST_TILE - 1) / INGEST_TILE;
  for (int64_t tile_id = blockIdx.x; tile_id < tiles_t * tiles_n; tile_id += gridDim.x) {
    const int64_t t0 = (tile_id / tiles_n) * INGEST_TILE, n0 = (tile_id % tiles_n) * INGEST_TILE;
    for (int r = ty; r < INGEST_TILE; r += 4) {
      const int64_t t = t0 + tx, n = n0 + r;
      if (t < rows && n < cols) tile[r][tx] = src[n * pitch + t];
    }
    __syncthreads();
    for (int r = ty; r < INGEST_TILE; r += 4) {
      const int64_t t = t0 + r, n = n0 + tx;
      if (t < rows && n < cols) dst[t * cols + n] = tile[tx][r];
    }
    __syncthreads();
  }
}

// any other pair of strides: one element per lane, the writes coalesced.  Rows over blockIdx.y, columns over x.
template <typename T>
__global__ void ingest_gather_kernel(const T* __restrict__ src, int64_t stride_t, int64_t stride_n, int64_t rows, int64_t cols,
                                     T* __restrict__ dst) {
  for (int64_t t = blockIdx.y; t < rows; t += gridDim.y) {
    const T* s = src + t * stride_t;
    T* d = dst + t * cols;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < cols; n += (int64_t)gridDim.x * blockDim.x) d[n] = s[n * stride_n];
  }
}

// The regime of a T x N view: a dimension of one element has no stride to speak of.
static inline int ingest_regime(int64_t T, int64_t N, int64_t stride_t, int64_t stride_n) {
  if (stride_n == 1 || N == 1) return INGEST_ROWS;
  if (stride_t == 1 || T == 1) return INGEST_TRANSPOSE;
  return INGEST_GATHER;
}

// dst (T x N, contiguous) = the view, on stream `st`; the caller checks the launch and synchronises
template <typename T_>
static void ingest_strided(hipStream_t st, const T_* src, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, T_* dst) {
  const int regime = ingest_regime(T, N, stride_t, stride_n);
  if (regime == INGEST_ROWS) {
    int64_t rows = T, cols = N, pitch = stride_t;
    if (pitch == cols || rows == 1) { cols *= rows; rows = 1; pitch = cols; }      // one contiguous run
    constexpr int V = 16 / (int)sizeof(T_);
    const int64_t bx = std::max<int64_t>(1, std::min<int64_t>((cols + (int64_t)EW_BLOCK * V - 1) / ((int64_t)EW_BLOCK * V), 4096));
    const dim3 grid((unsigned)bx, (unsigned)std::min<int64_t>(rows, 4096));
    hipLaunchKernelGGL((ingest_rows_kernel<T_>), grid, dim3(EW_BLOCK), 0, st, src, pitch, rows, cols, dst);
  } else if (regime == INGEST_TRANSPOSE) {
    const int64_t tiles = ((T + INGEST_TILE - 1) / INGEST_TILE) * ((N + INGEST_TILE - 1) / INGEST_TILE);
    hipLaunchKernelGGL((ingest_transpose_kernel<T_>), dim3((unsigned)std::min<int64_t>(tiles, (int64_t)1 << 20)), dim3(256), 0, st, src,
                       stride_n, T, N, dst);
  } else {
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((N + EW_BLOCK - 1) / EW_BLOCK, 4096)),
                    (unsigned)std::min<int64_t>(T, 4096));
    hipLaunchKernelGGL((ingest_gather_kernel<T_>), grid, dim3(EW_BLOCK), 0, st, src, stride_t, stride_n, T, N, dst);
  }
}

// out[t][:] = in[idx[t]][:]   (row resampling of a rows x cols matrix)
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ in, T* __restrict__ out, const int64_t* __restrict__ idx, int rows,
                                   int64_t cols) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / cols, c = i % cols;
    out[i] = in[idx[t] * cols + c];
  }
}

// out[t][j] = src(c[j])[t][local(c[j])] for t < rows, j < n_out: column resampling.  c = idx[j] indexes the columns of the virtual
// concatenation [left | right] of two row-major matrices with `rows` rows (right == nullptr, n_right == 0: left alone), so a
// column of `out` comes from either of them, each with its own leading dimension.  A workgroup owns a strip of GATHER_COLS_BLOCK
// output columns: every thread reads its index ONCE and resolves it to a column pointer and a stride, then walks a tile of
// GATHER_COLS_ROWS rows with them (blockIdx.y, grid-stride over the tiles) - stores are coalesced along j, loads are scattered
// inside one source row, GATHER_COLS_UNROLL of them in flight per thread, and the address of the next row is one add.  The
// workgroups of one row tile (consecutive blockIdx.x, dispatched together) read the same 32 source rows, 2.5 MB at 10 000 float64
// columns: the part of a cache line one strip does not use is found in L2 by the strip that does.
constexpr int GATHER_COLS_BLOCK = 256;
constexpr int GATHER_COLS_ROWS = 32;
constexpr int GATHER_COLS_UNROLL = 8;
template <typename T>
__global__ void __launch_bounds__(GATHER_COLS_BLOCK)
gather_concat_columns_kernel(const T* __restrict__ left, int64_t n_left, const T* __restrict__ right, int64_t n_right,
                             const int64_t* __restrict__ idx, T* __restrict__ out, int64_t n_out, int rows) {
  const int64_t j = (int64_t)blockIdx.x * GATHER_COLS_BLOCK + threadIdx.x;
  if (j >= n_out) return;
  const int64_t c = idx[j];
  const bool from_left = c < n_left;
  const int64_t ld = from_left ? n_left : n_right;
  const T* const col = from_left ? left + c : right + (c - n_left);
  for (int t0 = (int)blockIdx.y * GATHER_COLS_ROWS; t0 < rows; t0 += (int)gridDim.y * GATHER_COLS_ROWS) {
    const int t1 = t0 + GATHER_COLS_ROWS < rows ? t0 + GATHER_COLS_ROWS : rows;
    const T* s = col + (int64_t)t0 * ld;
    T* d = out + (int64_t)t0 * n_out + j;
    int t = t0;
    for (; t + GATHER_COLS_UNROLL <= t1; t += GATHER_COLS_UNROLL) {
      T v[GATHER_COLS_UNROLL];
#pragma unroll
      for (int u = 0; u < GATHER_COLS_UNROLL; ++u) v[u] = s[(int64_t)u * ld];
#pragma unroll
      for (int u = 0; u < GATHER_COLS_UNROLL; ++u) d[(int64_t)u * n_out] = v[u];
      s += (int64_t)GATHER_COLS_UNROLL * ld;
      d += (int64_t)GATHER_COLS_UNROLL * n_out;
    }
    for (; t < t1; ++t, s += ld, d += n_out) *d = *s;
  }
}

// grid of gather_concat_columns_kernel: one strip of columns per x, the row tiles over y (at most 65535 at a time)
static inline dim3 gather_cols_grid(int64_t rows, int64_t n_out) {
  int64_t by = (rows + GATHER_COLS_ROWS - 1) / GATHER_COLS_ROWS;
  if (by > 65535) by = 65535;
  if (by < 1) by = 1;
  return dim3((unsigned)((n_out + GATHER_COLS_BLOCK - 1) / GATHER_COLS_BLOCK), (unsigned)by);
}

// column sums and sums of squares of a rows x cols matrix: the column pass with one chunk, all the rows of a column in one thread
template <typename T>
struct ColumnMoments {
  const T* x; int64_t cols; double* sum; double* sumsq;
  __device__ void operator()(const ColChunk& k) const {
    double s = 0.0, q = 0.0;
    for (int r = k.r0; r < k.r1; ++r) {
      const double v = (double)x[(int64_t)r * cols + k.c];
      s += v;
      q += v * v;
    }
    sum[k.c] = s;
    sumsq[k.c] = q;
  }
};

// Pearson correlation from the raw cross products: r[n][j] = (C[n][j] - sx[n] sy[j] / T) / sqrt((qx[n] - sx[n]^2 / T) (qy[j] - sy[j]^2 / T)),
// clamped to [-1, 1] as numpy.corrcoef clips: C (GEMM) and qx, qy (column moments) sum in different orders, so a perfectly
// (anti-)correlated pair can land an ulp beyond 1.  The comparisons pass NaN through (fmin / fmax would not).
__global__ void pearson_finish_kernel(double* __restrict__ C, int64_t N, int m, int T, const double* __restrict__ sx,
                                      const double* __restrict__ qx, const double* __restrict__ sy, const double* __restrict__ qy) {
  const int64_t total = N * m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / m;
    const int j = (int)(i % m);
    const double cov = C[i] - sx[n] * sy[j] / T;
    const double vx = qx[n] - sx[n] * sx[n] / T, vy = qy[j] - sy[j] * sy[j] / T;
    const double r = cov / sqrt(vx * vy);          // constant columns give NaN, like numpy.corrcoef
    C[i] = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
  }
}

// Two-sided p-value of a Pearson correlation r of n_obs samples under the exact null distribution (tools/array.py:86-88):
// p = 2 I_x(a, a) with a = n_obs / 2 - 1 > 0 and x = (1 - |r|) / 2, the regularised incomplete beta function
//   I_x(a, a) = exp(a (ln x + ln(1 - x)) - ln a - ln B(a, a)) / cf(x),
// cf the continued fraction of I_x (DLMF 8.17.22) evaluated by the modified Lentz recurrence.  a = b puts x in [0, 1/2], the
// side on which the fraction converges, so there is no reflection.  x is formed from 1 - |r| (exact for |r| >= 1/2), never from
// 1 - r^2.  log_norm = -ln a - ln B(a, a) is the same for every value of a call and comes from the host (pvalue_log_norm).
// NaN stays NaN, |r| >= 1 is exactly 0, the result never exceeds 1, a prefactor below the normal range goes quietly to a
// denormal or 0.  The cap bounds the loop: a float64 run on the host needed at most 10 / 16 / 67 / 133 / 476 steps (at r near 0) for
// n_obs = 3 / 61 / 2920 / 20 000 / 10^6, and the entry points refuse an n_obs beyond PVALUE_MAX_OBS.
constexpr int PVALUE_MAX_STEPS = 1024;
constexpr int64_t PVALUE_MAX_OBS = 1000000;
__host__ __device__ inline double pearson_two_sided_p(const double r, const double a, const double log_norm) {
  if (r != r) return r;
  const double x = 0.5 * (1.0 - fabs(r));
  if (!(x > 0.0)) return 0.0;
  const double tiny = 1e-300, eps = 4.0 * 2.220446049250313e-16;
  const double a2 = a + a;
  double c = 1.0, d = 1.0 - a2 * x / (a + 1.0);
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= PVALUE_MAX_STEPS; ++m) {
    const double am = a + 2.0 * m;
    double t = m * (a - m) * x / ((am - 1.0) * am);           // even step
    d = 1.0 + t * d;
    c = 1.0 + t / c;
    if (fabs(d) < tiny) d = tiny;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    t = -(a + m) * (a2 + m) * x / (am * (am + 1.0));          // odd step
    d = 1.0 + t * d;
    c = 1.0 + t / c;
    if (fabs(d) < tiny) d = tiny;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= eps) break;
  }
  const double p = 2.0 * exp(a * (log(x) + log1p(-x)) + log_norm) * h;
  return p > 1.0 ? 1.0 : p;
}

// -ln a - ln B(a, a) = ln Gamma(2a) - 2 ln Gamma(a) - ln a for a = n_obs / 2 - 1 (host).  The three terms are about a ln a each
// and cancel to about 2 a ln 2, so they are taken in the host's extended precision and rounded once.
static inline double pvalue_log_norm(int64_t n_obs) {
  const long double a = (long double)n_obs / 2 - 1;
  return (double)(lgammal(2 * a) - 2 * lgammal(a) - logl(a));
}

// p[i] = pearson_two_sided_p(r[i])  (xmca_pearson_pvalues): one value per lane, lanes that converge early idle
__global__ void pearson_pvalues_kernel(const double* __restrict__ r, int64_t n, double a, double log_norm, double* __restrict__ p) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = pearson_two_sided_p(r[i], a, log_norm);
}

// Final layout of the correlation maps (xmca_correlation_maps): row j of the n_full x m outputs is row row_of[j] of the compact
// correlations C (row_of == nullptr: j itself), NaN in both maps where row_of[j] < 0.  r is rounded to the returned type TR and
// p computed from the rounded value, as the host route computes p from the r it returns.
template <typename TR>
__global__ void correlation_maps_kernel(const double* __restrict__ C, const int64_t* __restrict__ row_of, int64_t n_full, int m, double a,
                                        double log_norm, TR* __restrict__ r_out, double* __restrict__ p_out) {
  const int64_t total = n_full * m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i / m;
    const int64_t c = row_of ? row_of[j] : j;
    if (c < 0) {
      r_out[i] = (TR)__builtin_nan("");
      p_out[i] = __builtin_nan("");
      continue;
    }
    const TR r = (TR)C[c * m + (i - j * m)];
    r_out[i] = r;
    p_out[i] = pearson_two_sided_p((double)r, a, log_norm);
  }
}

// ------------------------------------------------------------------------------------------------
// Spatial maps in their final layout (xmca_get_maps): scaled / masked EOFs, amplitude and phase maps from the compact n x q values
// C that eof_mix_kernel / eof_transpose_kernel leave on the device (float64 whatever the output type - the statistics are those of
// the unrounded values, and a value that is only rounded at the end has the bits xmca_get_eofs returns; interleaved when `cc`).
// ------------------------------------------------------------------------------------------------
constexpr int MAP_EOF = 0, MAP_AMPLITUDE = 1, MAP_PHASE = 2;       // XMCA_MAP_* of the header
constexpr int STAT_MAX_RE = 0, STAT_MAX_AMP = 1, STAT_STD = 2;     // what a column is divided by
constexpr int MAP_STAT_BLOCKS = 1024;                              // most partials per column

// z = C[idx] * f: the per-column factor (fr, fi) is applied only when there is one (`hf`), so that values without a factor pass
// bit for bit; a real value with a real factor keeps im = +0 (atan2 then gives 0 or pi, as numpy does for a real array)
__device__ __forceinline__ void map_value(const double* __restrict__ C, bool cc, int64_t idx, bool hf, bool fc, double fr, double fi,
                                          double& re, double& im) {
  double vr, vi = 0.0;
  if (cc) { vr = C[2 * idx]; vi = C[2 * idx + 1]; }
  else vr = C[idx];
  if (!hf) { re = vr; im = vi; }
  else if (fc) { re = vr * fr - vi * fi; im = vr * fi + vi * fr; }
  else { re = vr * fr; im = cc ? vi * fr : 0.0; }
}

// (count, mean, M2) of two disjoint samples -> of their union (Chan, Golub & LeVeque 1983); an empty side changes nothing
__device__ __forceinline__ void moments_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
  const double n = na + nb;
  if (nb == 0.0) return;
  const double d = mb - ma, w = nb / n;
  ma += d * w;
  qa += qb + d * d * na * w;
  na = n;
}

// Partials of the column statistics: workgroup b reduces the rows b * 256 + t + k * 256 * gridDim.x of every column to ONE partial -
// the largest |Re z| or |z|, or the (count, mean, M2) of Re z - in part[(b * q + c) * NP .. + NP), NP = 3 for STAT_STD and 1
// otherwise.  One row per lane, 8 columns at a time in registers (the row's values lie side by side); every column is reduced over
// the 64 lanes of a wave by shuffles, then over the four waves through LDS.  No atomics: the same bits every call.  The moments are Welford's recurrence per lane and Chan's merge from there on, never E[x^2] - E[x]^2.
template <int STAT>
__global__ __launch_bounds__(256) void map_column_partials_kernel(const double* __restrict__ C, int cc, int64_t n, int q,
                                                                 const double* __restrict__ fr, const double* __restrict__ fi,
                                                                 double* __restrict__ part) {
  constexpr int NP = STAT == STAT_STD ? 3 : 1;
  __shared__ double red[4][8][NP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool hf = fr != nullptr, fc = fi != nullptr;
  for (int c0 = 0; c0 < q; c0 += 8) {
    double a0[8], a1[8], a2[8], pr[8], pi[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + u < q ? c0 + u : q - 1;
      a0[u] = a1[u] = a2[u] = 0.0;
      pr[u] = hf ? fr[c] : 1.0;
      pi[u] = fc ? fi[c] : 0.0;
    }
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u < q ? c0 + u : q - 1;
        double re, im;
        map_value(C, cc != 0, r * q + c, hf, fc, pr[u], pi[u], re, im);
        if constexpr (STAT == STAT_STD) {
          a0[u] += 1.0;
          const double d = re - a1[u];
          a1[u] += d / a0[u];
          a2[u] += d * (re - a1[u]);
        } else if constexpr (STAT == STAT_MAX_AMP) {
          a0[u] = fmax(a0[u], sqrt(re * re + im * im));
        } else {
          a0[u] = fmax(a0[u], fabs(re));
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        if constexpr (STAT == STAT_STD) {
          const double nb = __shfl_xor(a0[u], s, 64), mb = __shfl_xor(a1[u], s, 64), qb = __shfl_xor(a2[u], s, 64);
          // (both lanes of a pair merge the same two samples, the lower lane's first, so they agree bit for bit)
          if (lane & s) {
            double nn = nb, mm = mb, qq = qb;
            moments_merge(nn, mm, qq, a0[u], a1[u], a2[u]);
            a0[u] = nn; a1[u] = mm; a2[u] = qq;
          } else {
            moments_merge(a0[u], a1[u], a2[u], nb, mb, qb);
          }
        } else {
          a0[u] = fmax(a0[u], __shfl_xor(a0[u], s, 64));
        }
      }
      if (lane == 0) {
        red[wave][u][0] = a0[u];
        if constexpr (STAT == STAT_STD) { red[wave][u][1] = a1[u]; red[wave][u][2] = a2[u]; }
      }
    }
    __syncthreads();
    if (threadIdx.x < 8 && c0 + (int)threadIdx.x < q) {
      const int u = threadIdx.x;
      double* o = part + ((int64_t)blockIdx.x * q + c0 + u) * NP;
      if constexpr (STAT == STAT_STD) {
        double nn = red[0][u][0], mm = red[0][u][1], qq = red[0][u][2];
        for (int w = 1; w < 4; ++w) moments_merge(nn, mm, qq, red[w][u][0], red[w][u][1], red[w][u][2]);
        o[0] = nn; o[1] = mm; o[2] = qq;
      } else {
        o[0] = fmax(fmax(red[0][u][0], red[1][u][0]), fmax(red[2][u][0], red[3][u][0]));
      }
    }
    __syncthreads();
  }
}

// ... and their merge, in the order of the workgroups: div[c] = the maximum, or the population standard deviation sqrt(M2 / count)
template <int STAT>
__global__ void map_column_finish_kernel(const double* __restrict__ part, int blocks, int q, double* __restrict__ div) {
  constexpr int NP = STAT == STAT_STD ? 3 : 1;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= q) return;
  double nn = part[(int64_t)c * NP], mm = 0.0, qq = 0.0;
  if constexpr (STAT == STAT_STD) { mm = part[(int64_t)c * NP + 1]; qq = part[(int64_t)c * NP + 2]; }
  for (int b = 1; b < blocks; ++b) {
    const double* p = part + ((int64_t)b * q + c) * NP;
    if constexpr (STAT == STAT_STD) moments_merge(nn, mm, qq, p[0], p[1], p[2]);
    else nn = fmax(nn, p[0]);
  }
  div[c] = STAT == STAT_STD ? sqrt(qq / nn) : nn;
}

// Final layout: row j of the n_full x q output is row row_of[j] of C (row_of == nullptr: j itself) times the factor of its column,
// as value (MAP_EOF; interleaved complex when `oc`), sqrt(re^2 + im^2) or atan2(im, re), divided by div[c] (nullptr: as it is; a
// plain IEEE division, a zero column gives inf / NaN as on the host) and rounded to TO; NaN - in both planes - where row_of[j] < 0.
template <typename TO>
__global__ void map_finish_kernel(const double* __restrict__ C, int cc, const int64_t* __restrict__ row_of, int64_t n_full, int q,
                                  const double* __restrict__ fr, const double* __restrict__ fi, const double* __restrict__ div,
                                  int kind, int oc, TO* __restrict__ out) {
  const int64_t total = n_full * q;
  const bool hf = fr != nullptr, fc = fi != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i / q;
    const int c = (int)(i - j * q);
    const int64_t r = row_of ? row_of[j] : j;
    double re, im;
    if (r < 0) {
      re = im = __builtin_nan("");
    } else {
      map_value(C, cc != 0, r * q + c, hf, fc, hf ? fr[c] : 1.0, fc ? fi[c] : 0.0, re, im);
      if (kind == MAP_AMPLITUDE) re = sqrt(re * re + im * im);
      else if (kind == MAP_PHASE) re = atan2(im, re);
      if (div) { const double d = div[c]; re /= d; im /= d; }
    }
    if (oc) { out[2 * i] = (TO)re; out[2 * i + 1] = (TO)im; }
    else out[i] = (TO)re;
  }
}

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 counter-based generator (Salmon et al. 2011) -> standard normals (Box-Muller).
// counter = (element pair index lo, hi, run, side), key = seed: the stream of a surrogate depends only on
// (seed, run, side), never on which GPU generates it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

template <typename T>
__global__ void philox_normal_kernel(T* __restrict__ out, int64_t n, uint64_t seed, uint32_t run, uint32_t side) {
  const int64_t pairs = (n + 1) / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), run, side, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint64_t a = ((uint64_t)r[0] << 32) | r[1], b = ((uint64_t)r[2] << 32) | r[3];
    const double u1 = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);   // (0,1)
    const double u2 = ((double)(b >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    out[2 * i] = (T)(rad * cs);
    if (2 * i + 1 < n) out[2 * i + 1] = (T)(rad * sn);
  }
}

// ------------------------------------------------------------------------------------------------
// Red-noise surrogates: the AR(1) recurrence down the columns of the T x N plane of normals e that
// philox_normal_kernel has just filled, in place,
//   x[0] = e[0],   x[t] = fma(phi_c, x[t-1], sqrt(1 - phi_c^2) e[t]),
// in float64 whatever the plane's type (x is rounded on store, the state is not).  A lane per column, a row per step: every
// access is one coalesced row piece.  Columns alone leave the chip empty, so time is cut into segments that depend on
// (T, N) ONLY - never on lanes, ranks or occupancy: the surrogates must not depend on who makes them.
// ------------------------------------------------------------------------------------------------
constexpr int AR1_BLOCK = 64;           // one wave per workgroup: the grid spreads over the CUs at every width
constexpr int AR1_ROWS_IN_FLIGHT = 8;   // independent row loads issued ahead of the dependent FMA chain
constexpr int AR1_MIN_SEGMENT = 32;     // rows: a shorter segment is not worth its carry
constexpr int AR1_MAX_SEGMENTS = 64;
constexpr int AR1_TARGET_WAVES = 2048;  // 256 CUs x 8 waves

struct Ar1Segments {
  int64_t count, length;     // segment k covers the rows [k length, min(T, (k + 1) length))
};

// as many segments as fill the chip at this width, none shorter than AR1_MIN_SEGMENT rows (the last one excepted)
__host__ __device__ inline Ar1Segments ar1_segments(int64_t T, int64_t N) {
  const int64_t waves = (N + 63) / 64;
  int64_t want = (AR1_TARGET_WAVES + waves - 1) / waves;
  if (want > AR1_MAX_SEGMENTS) want = AR1_MAX_SEGMENTS;
  int64_t length = (T + want - 1) / want;
  if (length < AR1_MIN_SEGMENT) length = AR1_MIN_SEGMENT;
  return {(T + length - 1) / length, length};
}

// sqrt(1 - phi^2) as sqrt((1 - phi)(1 + phi)): no cancellation near |phi| = 1, and nothing the compiler may fuse
__device__ __forceinline__ double ar1_innovation_scale(double phi) { return sqrt((1.0 - phi) * (1.0 + phi)); }

__device__ __forceinline__ double ar1_ipow(double b, int64_t n) {
  double r = 1.0;
  for (; n > 0; n >>= 1, b *= b)
    if (n & 1) r *= b;
  return r;
}

// the rows [r0, r1) of column c from the state `prev` (the value of row r0 - 1; row 0 is e[0] itself): returns the value of row
// r1 - 1.  STORE: x is written over e.  The loads of a batch do not depend on the recurrence and are issued together.
template <typename T, bool STORE>
__device__ __forceinline__ double ar1_run(T* __restrict__ x, int64_t cols, int64_t c, int64_t r0, int64_t r1, double phi, double a,
                                          double prev) {
  int64_t r = r0;
  if (r == 0) {
    prev = (double)x[c];
    r = 1;
  }
  for (; r + AR1_ROWS_IN_FLIGHT <= r1; r += AR1_ROWS_IN_FLIGHT) {
    double e[AR1_ROWS_IN_FLIGHT];
#pragma unroll
    for (int j = 0; j < AR1_ROWS_IN_FLIGHT; ++j) e[j] = (double)x[(r + j) * cols + c];
#pragma unroll
    for (int j = 0; j < AR1_ROWS_IN_FLIGHT; ++j) {
      prev = fma(phi, prev, a * e[j]);
      if (STORE) x[(r + j) * cols + c] = (T)prev;
    }
  }
  for (; r < r1; ++r) {
    prev = fma(phi, prev, a * (double)x[r * cols + c]);
    if (STORE) x[r * cols + c] = (T)prev;
  }
  return prev;
}

// Pass A: carry[k][c] = the value the last row of segment k takes from a zero state in front of it (segment 0: its true value);
// grid (columns, segments - 1), the last segment hands nothing on.  Reads only.
template <typename T>
__global__ void ar1_carry_kernel(const T* __restrict__ e, int64_t rows, int64_t cols, int64_t seg_len, const double* __restrict__ phi,
                                 double* __restrict__ carry) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  const int64_t k = blockIdx.y, r0 = k * seg_len, r1 = min(rows, r0 + seg_len);
  const double p = phi[c], a = ar1_innovation_scale(p);
  carry[k * cols + c] = ar1_run<T, false>(const_cast<T*>(e), cols, c, r0, r1, p, a, 0.0);
}

// Pass B: the state in front of segment k in a fixed order, in_1 = carry_0, in_j = phi^len in_{j-1} + carry_{j-1}, then the
// segment is run again from it and stored: within a segment the bits are those of the sequential recurrence.  grid (columns,
// segments); `carry` may be null when there is one segment.
template <typename T>
__global__ void ar1_filter_kernel(T* __restrict__ x, int64_t rows, int64_t cols, int64_t seg_len, const double* __restrict__ phi,
                                  const double* __restrict__ carry) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  const int64_t k = blockIdx.y, r0 = k * seg_len, r1 = min(rows, r0 + seg_len);
  const double p = phi[c], a = ar1_innovation_scale(p);
  double in = 0.0;
  if (k > 0) {
    const double decay = ar1_ipow(p, seg_len);
    in = carry[c];
    for (int64_t j = 1; j < k; ++j) in = fma(decay, in, carry[j * cols + c]);
  }
  (void)ar1_run<T, true>(x, cols, c, r0, r1, p, a, in);
}

// ---------------------------------------------------------------------------------------------------------------------
// Leading rows of a product:  out (R x n, R <= 16) = A (R x K) B, float64, optionally row r times scale[r].
// The rotation behind a one-field solve reads 10 - 12 modes; the tiled GEMM spends a whole 128 x 128 tile's dependent chain
// (0.39 ms at K = 2920) on them whatever their number.  Here B is streamed once - a memory-bound pass - and A, 16 rows, comes
// through the scalar cache: the k index is uniform in a wave, every lane owns one output column and 16 sums.
//   KFAST = false:  B(k, j) = B[k * ldb + j]   (rows of the field: lanes along j read 512 contiguous bytes per k)
//   KFAST = true :  B(k, j) = B[j * ldb + k]   (rows of the eigenvector plane: a wave turns 64 columns x 32 k through LDS)
// The contraction is cut over the workgroups of grid.y (kchunk each, a multiple of LEAD_KSTEP) and inside a chunk over the four
// waves; the waves' sums are added in wave order, the chunks' in chunk order (lead_rows_sum_kernel): no atomics, and the same
// bits for the same shape from call to call.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LEAD_ROWS = 16;
constexpr int LEAD_COLS = 64;                        // output columns of a workgroup, one per lane
constexpr int LEAD_WAVES = 4;
constexpr int LEAD_KT = 32;                          // KFAST: k per wave and step
constexpr int LEAD_KSTEP = LEAD_WAVES * LEAD_KT;

template <bool KFAST>
__global__ __launch_bounds__(LEAD_WAVES * 64) void lead_rows_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ B,
                                                                    int64_t ldb, int R, int K, int n, int kchunk, double* __restrict__ out,
                                                                    int64_t ldo, const double* __restrict__ scale, double* __restrict__ part) {
  // KFAST: one 64 x 32 tile per wave, element (c, t) at [c * 32 + (t ^ (c & 31))] - the 32 lanes of a half-wave hit 32 different
  // bank pairs on the write (c fixed, t = lane) and on the read (t fixed, c = lane); 64 KiB.  Both: the waves' sums, [w][r][c].
  __shared__ double sh[KFAST ? LEAD_WAVES * LEAD_COLS * LEAD_KT : LEAD_WAVES * LEAD_ROWS * LEAD_COLS];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = blockIdx.x * LEAD_COLS;
  const int kb = blockIdx.y * kchunk, ke = min(K, kb + kchunk);       // (the grid has no empty chunk: kb < K)
  double acc[LEAD_ROWS];
  int ao[LEAD_ROWS];                                 // row r >= R repeats row R - 1 (its sums are dropped): A is never read outside R x K
#pragma unroll
  for (int r = 0; r < LEAD_ROWS; ++r) {
    acc[r] = 0.0;
    ao[r] = min(r, R - 1) * (int)lda;                // (lead_rows checks that A fits 32-bit offsets: scalar loads take one as it is)
  }
  if (KFAST) {
    double* tile = sh + w * (LEAD_COLS * LEAD_KT);
    const int kk = lane & 31, half = lane >> 5;
    for (int ks = kb; ks < ke; ks += LEAD_KSTEP) {
      const int k0 = ks + w * LEAD_KT;               // this wave's 32 k of the step (may lie behind ke: the tile is then not read)
      const int kc = min(k0 + kk, ke - 1);
      double v[LEAD_KT];
#pragma unroll
      for (int j = 0; j < LEAD_KT; ++j) v[j] = B[(int64_t)min(c0 + 2 * j + half, n - 1) * ldb + kc];
#pragma unroll
      for (int j = 0; j < LEAD_KT; ++j) {
        const int c = 2 * j + half;
        tile[c * LEAD_KT + (kk ^ (c & 31))] = v[j];
      }
      __syncthreads();
      const int tmax = max(0, min(LEAD_KT, ke - k0));
      for (int t = 0; t < tmax; ++t) {
        const double y = tile[lane * LEAD_KT + (t ^ (lane & 31))];
        const double* Ak = A + k0 + t;
#pragma unroll
        for (int r = 0; r < LEAD_ROWS; ++r) acc[r] = fma(Ak[ao[r]], y, acc[r]);
      }
      __syncthreads();
    }
  } else {
    const int per = kchunk / LEAD_WAVES;
    const int k0 = kb + w * per, k1 = min(ke, k0 + per);
    const double* Bc = B + min(c0 + lane, n - 1);    // (lanes behind the last column repeat it; their sums are dropped)
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
      double y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) y[u] = Bc[(int64_t)(k + u) * ldb];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double* Ak = A + k + u;
#pragma unroll
        for (int r = 0; r < LEAD_ROWS; ++r) acc[r] = fma(Ak[ao[r]], y[u], acc[r]);
      }
    }
    for (; k < k1; ++k) {
      const double y = Bc[(int64_t)k * ldb];
      const double* Ak = A + k;
#pragma unroll
      for (int r = 0; r < LEAD_ROWS; ++r) acc[r] = fma(Ak[ao[r]], y, acc[r]);
    }
  }
  // (KFAST: the loop ended on a barrier, the tiles are free)
#pragma unroll
  for (int r = 0; r < LEAD_ROWS; ++r) sh[(w * LEAD_ROWS + r) * LEAD_COLS + lane] = acc[r];
  __syncthreads();
  for (int o = threadIdx.x; o < LEAD_ROWS * LEAD_COLS; o += LEAD_WAVES * 64) {
    const int r = o / LEAD_COLS, col = c0 + o % LEAD_COLS;
    if (r >= R || col >= n) continue;
    double s = sh[o];
#pragma unroll
    for (int q = 1; q < LEAD_WAVES; ++q) s += sh[q * LEAD_ROWS * LEAD_COLS + o];
    if (part) part[((int64_t)blockIdx.y * R + r) * n + col] = s;
    else out[(int64_t)r * ldo + col] = scale ? s * scale[r] : s;
  }
}

// out[r][c] = scale[r] * (part[0][r][c] + part[1][r][c] + ...), the chunks in their order
__global__ void lead_rows_sum_kernel(const double* __restrict__ part, int chunks, int R, int n, double* __restrict__ out, int64_t ldo,
                                     const double* __restrict__ scale) {
  const int64_t cnt = (int64_t)R * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    double s = part[i];
    for (int q = 1; q < chunks; ++q) s += part[(int64_t)q * cnt + i];
    const int64_t r = i / n;
    out[r * ldo + (i - r * n)] = scale ? s * scale[r] : s;
  }
}

// The cut of the contraction depends on the shape alone: about three workgroups per CU of a 256-CU device where K allows it
// (B is read once whatever the cut; the chunks' sums cost ks * R * n doubles of traffic, <3 % of B at the shapes of a solve).
// The 768 is deliberately a constant and NOT the device's CU count: the cut fixes the order of the sums, and a result must
// not change its bits with the device (or the partition of one) it was computed on.
inline int lead_rows_chunk(int K, int n) {
  const int want = std::max(1, ceil_div(768, ceil_div(n, LEAD_COLS)));
  return ceil_div(ceil_div(K, want), LEAD_KSTEP) * LEAD_KSTEP;
}
// `part`: scratch for the chunks' sums, the caller's (it must stay until the stream has run the two kernels)
inline void lead_rows(hipStream_t st, bool b_kfast, const double* A, int64_t lda, const double* B, int64_t ldb, int R, int K, int n,
                      double* out, int64_t ldo, const double* scale, DevBuf<double>& part) {
  XMCA_CHECK(A && B && out && R >= 1 && R <= LEAD_ROWS && K >= 1 && n >= 1 && lda >= K && ldo >= n && ldb >= (b_kfast ? K : n) &&
                 lda * LEAD_ROWS < ((int64_t)1 << 28),
             XMCA_ERR_INVALID, "lead_rows: bad shape");
  const int kchunk = lead_rows_chunk(K, n), ks = ceil_div(K, kchunk);
  double* p = ks > 1 ? part.ensure((size_t)ks * R * n) : nullptr;
  const dim3 grid((unsigned)ceil_div(n, LEAD_COLS), (unsigned)ks);
  if (b_kfast) hipLaunchKernelGGL(lead_rows_kernel<true>, grid, dim3(LEAD_WAVES * 64), 0, st, A, lda, B, ldb, R, K, n, kchunk, out, ldo, scale, p);
  else hipLaunchKernelGGL(lead_rows_kernel<false>, grid, dim3(LEAD_WAVES * 64), 0, st, A, lda, B, ldb, R, K, n, kchunk, out, ldo, scale, p);
  if (ks > 1) hipLaunchKernelGGL(lead_rows_sum_kernel, ew_grid((int64_t)R * n), dim3(EW_BLOCK), 0, st, p, ks, R, n, out, ldo, scale);
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
