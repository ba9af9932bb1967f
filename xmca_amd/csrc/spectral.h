// Spectral maps: Welch power spectra of every column of a T x N field with missing values (NaN) and its cross-spectrum,
// coherence, phase and gain against q <= 4 gap-free index series, xmca_amd.spectral.spectral_maps.  With L = nperseg, segment m covers
// the rows m step .. m step + L - 1, m < K = (T - L) / step + 1 (scipy's layout with noverlap = L - step); it is present for column n
// exactly when its L entries are, K_n counts the present ones, and a missing value drops the segments that hold it and nothing else.
// With c_n the mean of the column's present values (0 with detrend = none) and x' = x - c_n, the segment DFT at bin k is
//   A_k = sum_j (w_j x'_j) (cos t - i sin t),  t = 2 pi ((k j) mod L) / L,
// the real and the imaginary part one float64 fma chain each in ascending j from +0.0, whatever the type of the field; (cos t, -sin t)
// come from a table of L entries the host built in extended precision, indexed by exact integer arithmetic - the device calls no
// sincos.  Z_k = A_k - mu W_k with mu = (sum_j x'_j) / L and W the DFT of the weights (a host table): the DFT of the de-meaned, windowed
// segment in one pass (mu = 0 with detrend = none).  Its energy e = P2 - mu (2 P1 - mu sum w^2), P2 = sum_j (w_j x'_j)^2,
// P1 = sum_j w_j (w_j x'_j), is sum_j (w_j (x'_j - mu))^2: by Parseval the mean of |Z_k|^2 over all L bins.  Over the present segments
// in ascending m:  Sxx_k = sum |Z|^2,  R = sum e,  and per series  Syy_k = sum |Y|^2,  C_k = sum conj(Y) Z,  Ry = sum e_y,  Y and e_y
// the same arithmetic on the index (spectral_index_kernel shares spectral_segment with the hot kernel: the two sides cannot drift
// apart).  A segment that is not present adds +0.0 to every chain.  No atomic, no scratch memory, no mask or widened plane; a gap
// is recognised on load by v == v.  A call repeats its bits, and the chains of a bin are its own: its maps depend neither on the
// other bins of the call nor on their order.
#pragma once
#include <cmath>
#include <vector>

#include "lead_lag.h"

namespace xmca {

constexpr int SP_COLS = 256;                     // columns of a workgroup: one lane each (xmca_spectral_tile)
constexpr int SP_ROWS = 8;                       // rows of a piece: the loads a lane keeps in flight
constexpr int SP_MAX_Q = 4;                      // most index series
constexpr int SP_MIN_L = 8, SP_MAX_L = 4096;     // nperseg
constexpr double SP_LIVE = 0x1p-40;              // a bin carries power when Sxx > SP_LIVE R (and Syy > SP_LIVE Ry)

// bins of a group per number of index series: 2 B accumulators of the segment and B (1 + 3 Q) over the segments in a lane's
// registers, chosen from the register report
__host__ __device__ constexpr int sp_group(int q) { return q == 0 ? 8 : q == 1 ? 8 : q == 2 ? 6 : q == 3 ? 4 : 3; }
// values per (bin, column) of the sums plane: Sxx and per index series Syy, Re C, Im C
__host__ __device__ constexpr int sp_sums(int q) { return 1 + 3 * q; }

// (cos t, -sin t), t = 2 pi i / L, in extended precision and rounded once: the angle is folded into [0, pi / 4] by integer
// arithmetic, so the entries at the multiples of a quarter turn are exact.
static inline void sp_twiddle(int i, int L, double* c_out, double* ms_out) {
  int64_t a = 4 * (int64_t)i;                    // in units of 2 pi / (4 L); 0 <= a < 4 L
  int ss = 1, cs = 1;
  if (a > 2 * (int64_t)L) { a = 4 * (int64_t)L - a; ss = -1; }
  if (a > L) { a = 2 * (int64_t)L - a; cs = -1; }
  const bool swap = 2 * a > L;
  if (swap) a = L - a;
  const long double t = 3.14159265358979323846264338327950288L * (long double)a / (long double)(2 * (int64_t)L);
  long double c = cosl(t), s = sinl(t);
  if (swap) { const long double k = c; c = s; s = k; }
  *c_out = (double)(cs * c);
  *ms_out = (double)(-(ss * s));
}

// The host tables of a call: tw (cos, -sin) interleaved at i < L; W (Re, Im) of the DFT of the weights at the F bins and sum w^2, both
// ascending sums in extended precision rounded once; Ke[K], K = 0 .. k_max (Welch 1967):
// Ke = K / (1 + 2 sum_{j >= 1, j step < L, j < K} (1 - j / K) rho_j^2), rho_j = sum_i w_i w_{i + j step} / sum w^2; Ke[0] = 0.
static inline void sp_tables(const double* w, int L, int step, const int* bins, int F, int k_max, std::vector<double>& tw, std::vector<double>& W,
                             double* w2_out, std::vector<double>& Ke) {
  tw.resize(2 * (size_t)L);
  for (int i = 0; i < L; ++i) sp_twiddle(i, L, &tw[2 * (size_t)i], &tw[2 * (size_t)i + 1]);
  long double w2 = 0.0L;
  for (int i = 0; i < L; ++i) w2 += (long double)w[i] * (long double)w[i];
  *w2_out = (double)w2;
  W.resize(2 * (size_t)F);
  for (int f = 0; f < F; ++f) {
    long double re = 0.0L, im = 0.0L;
    int idx = 0;
    for (int j = 0; j < L; ++j) {
      re += (long double)w[j] * (long double)tw[2 * (size_t)idx];
      im += (long double)w[j] * (long double)tw[2 * (size_t)idx + 1];
      idx += bins[f];
      if (idx >= L) idx -= L;
    }
    W[2 * (size_t)f] = (double)re;
    W[2 * (size_t)f + 1] = (double)im;
  }
  std::vector<long double> rho2;
  for (int j = 1; (int64_t)j * step < L; ++j) {
    long double s = 0.0L;
    for (int i = 0; i + j * step < L; ++i) s += (long double)w[i] * (long double)w[i + j * step];
    rho2.push_back((s / w2) * (s / w2));
  }
  Ke.assign((size_t)k_max + 1, 0.0);
  for (int K = 1; K <= k_max; ++K) {
    long double den = 1.0L;
    for (int j = 1; j <= (int)rho2.size() && j < K; ++j) den += 2.0L * (1.0L - (long double)j / (long double)K) * rho2[(size_t)j - 1];
    Ke[(size_t)K] = (double)((long double)K / den);
  }
}

// One segment of one column at the B bins k[.]: the chains of the header comment.  `col` is the lane's column (stride N), row0 the
// first row of the segment; tw (cos, -sin) and w are the tables in LDS, their offsets idx[b] = (k[b] j) mod L uniform over the
// workgroup and stepped by exact integer arithmetic (k[b] <= L / 2 < L: one subtraction).  The rows come in pieces of SP_ROWS whose
// loads are issued together; no branch surrounds a load: a row past the segment reads its last row and counts for nothing.
// Bounds: rows row0 .. row0 + L - 1 of the column (the caller's row0 + L <= T); tw, w at [0, L).
template <typename TI, int B>
__device__ __forceinline__ void spectral_segment(const TI* __restrict__ col, int64_t N, double c, int64_t row0, int L, const int (&k)[B],
                                                 const double2* __restrict__ tw, const double* __restrict__ w, double (&re)[B], double (&im)[B],
                                                 double& s, double& p1, double& p2, bool& all_present) {
  constexpr int R = SP_ROWS;
  int idx[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    re[b] = im[b] = 0.0;
    idx[b] = 0;
  }
  s = p1 = p2 = 0.0;
  all_present = true;
  for (int j0 = 0; j0 < L; j0 += R) {
    TI v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int j = j0 + i < L ? j0 + i : L - 1;
      v[i] = col[(row0 + j) * N];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const bool inside = j0 + i < L;                        // (uniform)
      const int j = inside ? j0 + i : L - 1;
      const bool present = v[i] == v[i];
      all_present = all_present && (present || !inside);
      const double x = inside && present ? (double)v[i] - c : 0.0;
      const double wj = w[j];
      const double wx = wj * x;
      s += x;
      p1 = fma(wj, wx, p1);
      p2 = fma(wx, wx, p2);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const double2 t = tw[idx[b]];
        re[b] = fma(wx, t.x, re[b]);
        im[b] = fma(wx, t.y, im[b]);
        const int next = idx[b] + k[b];                      // (past the segment the offsets are not used again)
        idx[b] = next >= L ? next - L : next;
      }
    }
  }
}

// The energy of a segment, sum_j (w_j (x'_j - mu))^2 = P2 - mu (2 P1 - mu sum w^2), in this order on both sides.
__device__ __forceinline__ double sp_energy(double p1, double p2, double mu, double w2) { return fma(-mu, fma(-mu, w2, 2.0 * p1), p2); }

// The tables of a workgroup into LDS: tw at [0, L), w behind it.  Every thread of the workgroup takes part.
__device__ __forceinline__ void spectral_stage(const double2* __restrict__ tw_g, const double* __restrict__ w_g, int L, double2* tw, double* w) {
  for (int i = (int)threadIdx.x; i < L; i += (int)blockDim.x) {
    tw[i] = tw_g[i];
    w[i] = w_g[i];
  }
  __syncthreads();
}

// 1. The index side: Y[m][f][j] = Z of segment m of series j at bin f (Re, Im) and ey[m][j] its energy - spectral_segment on the
// T x Q plane of the centred index (c = 0: the host centred it), one lane per series, blockIdx.x the segment, blockIdx.y the
// group of bins.  Bounds: Yc at rows < T (m step + L <= T), columns j < Q; bins, W at f < F; Y at ((m F + f) Q + j); ey at (m Q + j).
template <int B>
__global__ __launch_bounds__(64) void spectral_index_kernel(const double* __restrict__ Yc, int Q, int L, int step, int demean,
                                                            const double2* __restrict__ tw_g, const double* __restrict__ w_g, double w2,
                                                            const int* __restrict__ bins, const double2* __restrict__ W, int F,
                                                            double2* __restrict__ Y, double* __restrict__ ey) {
  extern __shared__ double2 sp_lds[];
  double2* tw = sp_lds;
  double* w = reinterpret_cast<double*>(sp_lds + L);
  spectral_stage(tw_g, w_g, L, tw, w);
  const int lane = (int)threadIdx.x;
  const int j = lane < Q ? lane : Q - 1;                     // (a spare lane repeats the last series and writes nothing)
  const int m = (int)blockIdx.x;
  const int f0 = (int)blockIdx.y * B;
  int k[B];
#pragma unroll
  for (int b = 0; b < B; ++b) k[b] = bins[f0 + b < F ? f0 + b : F - 1];
  double re[B], im[B], s, p1, p2;
  bool all_present;
  spectral_segment<double, B>(Yc + j, Q, 0.0, (int64_t)m * step, L, k, tw, w, re, im, s, p1, p2, all_present);
  const double mu = demean ? s / (double)L : 0.0;
  if (lane >= Q) return;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    if (f0 + b < F) {
      const double2 Wk = W[f0 + b];
      Y[((int64_t)m * F + f0 + b) * Q + j] = make_double2(fma(-mu, Wk.x, re[b]), fma(-mu, Wk.y, im[b]));
    }
  }
  if (blockIdx.y == 0) ey[(int64_t)m * Q + j] = sp_energy(p1, p2, mu, w2);
}

// 2. The sums over the segments, the hot path.  A workgroup owns SP_COLS columns x one group of B bins (blockIdx.y; the last group
// may be partial: its spare slots repeat the last bin of the call and are not written).  A lane owns one column and keeps in
// registers the 2 B accumulators of the current segment with its three sums and present flag, and the B (1 + 3 Q) accumulators over
// the segments with K_n, R and Ry.  Overlapping segments re-read their rows.  The index spectra Y[m][f][.] and energies ey[m][.] are
// the same for the whole workgroup: wave-uniform loads.  A segment that is not present enters with Z = 0 and one = 0: it adds +0.0
// to every chain (the chains start from +0.0 and the index is finite, so the zeros leave their bits alone).  A lane past the last
// column repeats column N - 1 and writes nothing.  The group with blockIdx.y == 0 writes K_n, R and Ry.
// Bounds: X at rows < T (m step + L <= T for m < K), columns n < N; cn at n < N; bins, W at f < F; Y at ((m F + f) Q + j), ey at
// (m Q + j), m < K; sums at ((f S + i) N + n), S = 1 + 3 Q, i < S, f < F; seg at n; rr at (i N + n), i <= Q.
template <typename TI, int Q, int B>
__global__ __launch_bounds__(SP_COLS) void spectral_segments_kernel(const TI* __restrict__ X, int64_t N, const double* __restrict__ cn, int L, int step,
                                                                    int K, int demean, const double2* __restrict__ tw_g, const double* __restrict__ w_g,
                                                                    double w2, const int* __restrict__ bins, const double2* __restrict__ W, int F,
                                                                    const double2* __restrict__ Y, const double* __restrict__ ey,
                                                                    double* __restrict__ sums, int* __restrict__ seg, double* __restrict__ rr) {
  constexpr int S = sp_sums(Q);
  extern __shared__ double2 sp_lds[];
  double2* tw = sp_lds;
  double* w = reinterpret_cast<double*>(sp_lds + L);
  spectral_stage(tw_g, w_g, L, tw, w);
  const int64_t n_lane = (int64_t)blockIdx.x * SP_COLS + threadIdx.x;
  const int64_t n = n_lane < N ? n_lane : N - 1;
  const int f0 = (int)blockIdx.y * B;
  int k[B];
  double2 Wk[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int f = f0 + b < F ? f0 + b : F - 1;
    k[b] = bins[f];
    Wk[b] = W[f];
  }
  double sxx[B], syy[B][Q > 0 ? Q : 1], cre[B][Q > 0 ? Q : 1], cim[B][Q > 0 ? Q : 1], ry[Q > 0 ? Q : 1];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    sxx[b] = 0.0;
#pragma unroll
    for (int j = 0; j < Q; ++j) syy[b][j] = cre[b][j] = cim[b][j] = 0.0;
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) ry[j] = 0.0;
  double r = 0.0;
  int kn = 0;
  const TI* col = X + n;
  const double c = cn[n];
  for (int m = 0; m < K; ++m) {
    double re[B], im[B], s, p1, p2;
    bool all_present;
    spectral_segment<TI, B>(col, N, c, (int64_t)m * step, L, k, tw, w, re, im, s, p1, p2, all_present);
    const double mu = demean ? s / (double)L : 0.0;
    const double one = all_present ? 1.0 : 0.0;
    kn += all_present ? 1 : 0;
    r += all_present ? sp_energy(p1, p2, mu, w2) : 0.0;
#pragma unroll
    for (int j = 0; j < Q; ++j) ry[j] += one * ey[(int64_t)m * Q + j];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const double zr = all_present ? fma(-mu, Wk[b].x, re[b]) : 0.0;
      const double zi = all_present ? fma(-mu, Wk[b].y, im[b]) : 0.0;
      sxx[b] += fma(zi, zi, zr * zr);
      const int f = f0 + b < F ? f0 + b : F - 1;
      const double2* yrow = Y + ((int64_t)m * F + f) * Q;
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const double2 y = yrow[j];                           // (scalar registers)
        syy[b][j] += one * fma(y.y, y.y, y.x * y.x);
        cre[b][j] += fma(y.y, zi, y.x * zr);                 // conj(Y) Z = (yr zr + yi zi) + i (yr zi - yi zr)
        cim[b][j] += fma(-y.y, zr, y.x * zi);
      }
    }
  }
  if (n_lane >= N) return;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    if (f0 + b < F) {
      double* o = sums + (int64_t)(f0 + b) * S * N + n;
      o[0] = sxx[b];
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        o[(int64_t)(1 + 3 * j) * N] = syy[b][j];
        o[(int64_t)(2 + 3 * j) * N] = cre[b][j];
        o[(int64_t)(3 + 3 * j) * N] = cim[b][j];
      }
    }
  }
  if (blockIdx.y == 0) {
    seg[n] = kn;
    rr[n] = r;
#pragma unroll
    for (int j = 0; j < Q; ++j) rr[(int64_t)(1 + j) * N + n] = ry[j];
  }
}

// 3. The finish: one lane per entry (bin, column, series) - with Q = 0 per (bin, column) - in the final (F, N) / (F, N, q) layout.
// scale = side / (fs sum w^2 K_n), side = 1 at bin 0 and at bin L / 2 of an even L, else 2.  A column with K_n < min_segments (or
// none) is NaN in every map.  power = scale Sxx, index_power = scale Syy, cospectrum = scale Re C, quadrature = scale Im C.  The
// ratios are live when K_n >= 2, Sxx > 2^-40 R and Syy > 2^-40 Ry (a definition: an exactly constant column, and bin 0 of
// segments de-meaned under the boxcar, carry no power); else NaN.  coherence = |C|^2 / (Sxx Syy) clamped to [0, 1] by comparisons and rounded once to TR, phase =
// atan2(Im C, Re C), gain = |C| / Syy, p = exp((Ke[K_n] - 1) log1p(-coherence)) from the rounded coherence, 0 where that is 1.
// Bounds: seg at n < N; sums, rr as above; Ke at K_n <= K; bins at f < F; the outputs at i < F N (power) and i < F N q.
template <typename TR>
__global__ void spectral_finish_kernel(const double* __restrict__ sums, const int* __restrict__ seg, const double* __restrict__ rr,
                                       const double* __restrict__ Ke, const int* __restrict__ bins, int64_t N, int q, int F, int L, double fs,
                                       double w2, int min_segments, TR* __restrict__ power, TR* __restrict__ ipower, TR* __restrict__ co,
                                       TR* __restrict__ quad, TR* __restrict__ coh, TR* __restrict__ phase, TR* __restrict__ gain,
                                       double* __restrict__ p_out) {
  const int qq = q > 0 ? q : 1;
  const int64_t total = (int64_t)F * N * qq;
  const int S = sp_sums(q);
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t fn = i / qq;
    const int j = (int)(i - fn * qq);
    const int64_t f = fn / N, n = fn - f * N;
    const int kn = seg[n];
    const int k = bins[f];
    const double side = (k == 0 || 2 * k == L) ? 1.0 : 2.0;
    const double scale = side / (fs * w2 * (double)kn);
    const double* o = sums + f * S * N + n;
    const double sxx = o[0];
    const bool col_live = kn >= min_segments && kn >= 1;
    if (j == 0) power[fn] = col_live ? (TR)(scale * sxx) : (TR)nan;
    if (q == 0) continue;
    const double syy = o[(int64_t)(1 + 3 * j) * N], cr = o[(int64_t)(2 + 3 * j) * N], ci = o[(int64_t)(3 + 3 * j) * N];
    ipower[i] = col_live ? (TR)(scale * syy) : (TR)nan;
    co[i] = col_live ? (TR)(scale * cr) : (TR)nan;
    quad[i] = col_live ? (TR)(scale * ci) : (TR)nan;
    const bool live = col_live && kn >= 2 && sxx > SP_LIVE * rr[n] && syy > SP_LIVE * rr[(int64_t)(1 + j) * N + n];
    if (!live) {
      coh[i] = (TR)nan;
      phase[i] = (TR)nan;
      gain[i] = (TR)nan;
      p_out[i] = nan;
      continue;
    }
    const double c2 = fma(ci, ci, cr * cr);
    double g = c2 / (sxx * syy);
    g = g > 1.0 ? 1.0 : (g < 0.0 ? 0.0 : g);
    const TR gr = (TR)g;
    coh[i] = gr;
    phase[i] = (TR)atan2(ci, cr);
    gain[i] = (TR)(sqrt(c2) / syy);
    p_out[i] = (double)gr >= 1.0 ? 0.0 : exp((Ke[kn] - 1.0) * log1p(-(double)gr));
  }
}

// The launches on stream `st`.  LDS of a workgroup: the (cos, -sin) table and the weights, 24 L bytes - 96 KiB at L = 4096, above the
// 64 KiB a kernel may take without asking.
inline size_t sp_lds_bytes(int L) { return (size_t)L * (sizeof(double2) + sizeof(double)); }

template <int B>
static inline void spectral_index_b(hipStream_t st, const double* Yc, int q, int L, int step, int K, int demean, const double2* tw, const double* w,
                                    double w2, const int* bins, const double2* W, int F, double2* Y, double* ey) {
  const size_t lds = sp_lds_bytes(L);
  XMCA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spectral_index_kernel<B>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((spectral_index_kernel<B>), dim3((unsigned)K, (unsigned)ceil_div(F, B)), dim3(64), lds, st, Yc, q, L, step, demean, tw, w, w2,
                     bins, W, F, Y, ey);
}

static inline void spectral_index(hipStream_t st, const double* Yc, int q, int L, int step, int K, int demean, const double2* tw, const double* w,
                                  double w2, const int* bins, const double2* W, int F, double2* Y, double* ey) {
  switch (sp_group(q)) {          // (the group of the hot kernel with this q: the same instantiation of spectral_segment)
    case 8: spectral_index_b<8>(st, Yc, q, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey); break;
    case 6: spectral_index_b<6>(st, Yc, q, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey); break;
    case 4: spectral_index_b<4>(st, Yc, q, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey); break;
    case 3: spectral_index_b<3>(st, Yc, q, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey); break;
    default: throw Error(XMCA_ERR_INVALID, "spectral_maps: no index kernel for this group of bins");
  }
  XMCA_HIP(hipGetLastError());
}

template <typename TI, int Q>
static inline void spectral_segments_q(hipStream_t st, const TI* X, int64_t N, const double* cn, int L, int step, int K, int demean, const double2* tw,
                                       const double* w, double w2, const int* bins, const double2* W, int F, const double2* Y, const double* ey,
                                       double* sums, int* seg, double* rr) {
  constexpr int B = sp_group(Q);
  const size_t lds = sp_lds_bytes(L);
  XMCA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&spectral_segments_kernel<TI, Q, B>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  const dim3 grid((unsigned)ceil_div(N, SP_COLS), (unsigned)ceil_div(F, B));
  hipLaunchKernelGGL((spectral_segments_kernel<TI, Q, B>), grid, dim3(SP_COLS), lds, st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey,
                     sums, seg, rr);
}

template <typename TI>
static inline void spectral_segments(hipStream_t st, const TI* X, int64_t N, const double* cn, int q, int L, int step, int K, int demean,
                                     const double2* tw, const double* w, double w2, const int* bins, const double2* W, int F, const double2* Y,
                                     const double* ey, double* sums, int* seg, double* rr) {
  switch (q) {
    case 0: spectral_segments_q<TI, 0>(st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey, sums, seg, rr); break;
    case 1: spectral_segments_q<TI, 1>(st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey, sums, seg, rr); break;
    case 2: spectral_segments_q<TI, 2>(st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey, sums, seg, rr); break;
    case 3: spectral_segments_q<TI, 3>(st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey, sums, seg, rr); break;
    case 4: spectral_segments_q<TI, 4>(st, X, N, cn, L, step, K, demean, tw, w, w2, bins, W, F, Y, ey, sums, seg, rr); break;
    default: throw Error(XMCA_ERR_INVALID, "spectral_maps: between 0 and 4 index series are supported");
  }
  XMCA_HIP(hipGetLastError());
}

}  // namespace xmca
