// Bootstrap statistics of the singular vectors: the k leading vectors of a replicate are aligned with the
// model's, their deviation from the model's vectors is accumulated per lane in float64, and the lanes are merged into the
// bootstrap mean and standard error of every grid point.  Four streaming kernels; a replicate's vectors are read twice (dot,
// accumulate), the model's twice, the lane's accumulators are read and written once.  No atomics anywhere: every sum has a
// fixed order, so a call gives the same bits whenever the runs fall on the same lanes.
#pragma once
#include "kernels.h"

namespace xmca {

constexpr int PATTERN_BLOCK = 256;
// columns per partial sum of the alignment: a constant, so the association of the dot products is a function of N alone
// (xmca_pattern_tile)
constexpr int PATTERN_TILE = 1024;

static inline int64_t pattern_tiles(int64_t N) { return (N + PATTERN_TILE - 1) / PATTERN_TILE; }

// Partial c_j = sum_n conj(v0[j, n]) v[j, n] over the columns of one tile of one side: grid (tiles of the side, k), lanes along n.
// part: k x total_tiles pairs (re, im); this side's tiles start at tile_off.  v0: float64 planes, row stride ld0; v: planes of
// TV, row stride ldv (im planes nullptr: real).  Every (mode, tile) pair of the side is written, so `part` needs no clearing.
template <typename TV>
__global__ __launch_bounds__(PATTERN_BLOCK) void pattern_dot_partial_kernel(const double* __restrict__ v0_re, const double* __restrict__ v0_im,
                                                                            int64_t ld0, const TV* __restrict__ v_re,
                                                                            const TV* __restrict__ v_im, int64_t ldv, int64_t N,
                                                                            int tile_off, int total_tiles, double* __restrict__ part) {
  __shared__ double red[4];
  const int j = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * PATTERN_TILE;
  const int64_t end = begin + PATTERN_TILE < N ? begin + PATTERN_TILE : N;
  double cr = 0.0, ci = 0.0;
  for (int64_t n = begin + threadIdx.x; n < end; n += PATTERN_BLOCK) {
    const double a = v0_re[j * ld0 + n], x = (double)v_re[j * ldv + n];
    cr = fma(a, x, cr);
    if (v0_im) {
      const double b = v0_im[j * ld0 + n], y = (double)v_im[j * ldv + n];
      cr = fma(b, y, cr);
      ci += a * y - b * x;
    }
  }
  cr = block_sum_256(cr, red);
  if (v0_im) ci = block_sum_256(ci, red);
  if (threadIdx.x == 0) {
    double* p = part + 2 * ((int64_t)j * total_tiles + tile_off + blockIdx.x);
    p[0] = cr;
    p[1] = ci;
  }
}

// c_j = the tiles of the left side, then those of the right, added in that order; u_j = conj(c_j) / |c_j| (1 where c_j = 0; +-1
// for real vectors) to u (k pairs), the congruence |c_j| / n_fields to g (k values).  One thread per mode.
__global__ void pattern_phase_kernel(const double* __restrict__ part, int total_tiles, int k, int n_fields, double* __restrict__ u,
                                     double* __restrict__ g) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double cr = 0.0, ci = 0.0;
  for (int t = 0; t < total_tiles; ++t) {
    cr += part[2 * ((int64_t)j * total_tiles + t)];
    ci += part[2 * ((int64_t)j * total_tiles + t) + 1];
  }
  const double mag = ci == 0.0 ? fabs(cr) : hypot(cr, ci);
  u[2 * j] = mag > 0.0 ? cr / mag : 1.0;
  u[2 * j + 1] = mag > 0.0 ? -ci / mag : 0.0;
  g[j] = mag / (double)n_fields;
}

// d = u_j v[j, n] - v0[j, n]; S += d, Q += |d|^2 in the accumulators of the calling lane (k x N planes, S_im only for complex
// vectors): plain read-modify-write, ordered by the lane's stream.  Grid (ceil(N / block), k).
template <typename TV>
__global__ __launch_bounds__(PATTERN_BLOCK) void pattern_accumulate_kernel(const double* __restrict__ v0_re, const double* __restrict__ v0_im,
                                                                           int64_t ld0, const TV* __restrict__ v_re,
                                                                           const TV* __restrict__ v_im, int64_t ldv, int64_t N,
                                                                           const double* __restrict__ u, double* __restrict__ S_re,
                                                                           double* __restrict__ S_im, double* __restrict__ Q) {
  const int j = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * PATTERN_BLOCK + threadIdx.x;
  if (n >= N) return;
  const double ur = u[2 * j], ui = u[2 * j + 1];
  const double x = (double)v_re[j * ldv + n];
  const int64_t e = (int64_t)j * N + n;
  if (v0_im) {
    const double y = (double)v_im[j * ldv + n];
    const double dr = ur * x - ui * y - v0_re[j * ld0 + n], di = ur * y + ui * x - v0_im[j * ld0 + n];
    S_re[e] += dr;
    S_im[e] += di;
    Q[e] += dr * dr + di * di;
  } else {
    const double dr = ur * x - v0_re[j * ld0 + n];
    S_re[e] += dr;
    Q[e] += dr * dr;
  }
}

// The accumulators of the lanes, added in lane order: mean = v0 + S / R, std = sqrt(max(0, Q - |S|^2 / R) / (R - 1)).  acc holds
// lanes x ncomp planes of kN elements (S_re, S_im when complex, Q); mean: kN values, interleaved (re, im) when complex.
__global__ void pattern_merge_kernel(const double* __restrict__ acc, int lanes, int cplx, int64_t kN, const double* __restrict__ v0_re,
                                     const double* __restrict__ v0_im, double R, double* __restrict__ mean, double* __restrict__ std_out) {
  const int ncomp = cplx ? 3 : 2;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < kN; e += (int64_t)gridDim.x * blockDim.x) {
    double sr = 0.0, si = 0.0, q = 0.0;
    for (int l = 0; l < lanes; ++l) {
      const double* a = acc + (int64_t)l * ncomp * kN;
      sr += a[e];
      if (cplx) si += a[kN + e];
      q += a[(int64_t)(ncomp - 1) * kN + e];
    }
    if (cplx) {
      mean[2 * e] = v0_re[e] + sr / R;
      mean[2 * e + 1] = v0_im[e] + si / R;
    } else {
      mean[e] = v0_re[e] + sr / R;
    }
    std_out[e] = sqrt(fmax(0.0, q - (sr * sr + si * si) / R) / (R - 1.0));
  }
}

}  // namespace xmca
