// Hermitian eigensolver for the small (T x T or N x N) stage of solve():
// two-sided BLOCK Jacobi in f64 with round-robin pair slots (NT x NT tiles: 64 real, 32 complex).
//
//   per round, ONE launch (jacobi_fused_round_kernel; problems of one or two pair slots use the plain
//   jacobi_tile_evd_kernel + jacobi_update_kernel pair):
//     * tile solve - the first S workgroups assemble the diagonal tiles of the NEXT round from this round's inputs
//       (jacobi_assemble_next_diag) and sweep them once with a parallel-order cyclic Jacobi held in LDS
//       (jacobi_tile_evd_body; two-level form jacobi_cross_sweep_twolevel for the 64 x 64 real tiles).  Rotations
//       start from the identity and always take the inner angle, so the accumulated J_P stays close to the identity
//       -> quadratic outer convergence;
//     * update - all workgroups (the first S too, once done) process G'[P,Q] = J_P^H G[P,Q] J_Q (upper triangle, each
//       quarter written once in its upper orientation) and Z'[P,c] = J_P^H Z[P,c] on the f64 matrix pipe
//       (v_mfma_f64_16x16x4_f64) as statically assigned, software-pipelined work items (jacobi_persistent_update),
//       written straight to the slots of the NEXT round (ping-pong buffers), so the tournament permutation costs no
//       extra pass.
//   after 2S-1 rounds every pair of half-blocks has met once (= one sweep); jacobi_offmax_kernel decides when to stop.
//
// Z accumulates Q^H: at the end row i of Z is the conjugated eigenvector i.
// The kernels are in jacobi_kernels.h; this file holds the workspace, the host driver of the sweeps (jacobi_evd) and the
// entry point that chooses between them and the tridiagonal route (hermitian_evd).
// Replaces the LAPACK *gesdd calls of xmca/array.py:479 and :570.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "gemm.h"
#include "cholesky.h"
#include "tridiag.h"
#include "tridiag_vec.h"
#include "jacobi_kernels.h"

namespace xmca {

struct EvdInfo {
  int sweeps = 0;
  int tile = 0;
  int slots = 0;
  double last_off = 0.0;
  int lr_step = 0;        // 1: a Cholesky LR step was inserted (graded spectrum)
  double diag_spread = 0; // q10/q90 of the diagonal when that was decided
  int tridiag = 0;        // 1: solved by reduction to tridiagonal form (tridiag.h), no Jacobi sweeps
  int n_eigvec = 0;       // eigenvectors actually formed: 0 (values only), n, or the k' of the partial route (hermitian_evd)
};

struct EvdWorkspace {
  DevBuf<double> G[2][2], Z[2][2];   // [ping-pong][plane]
  DevBuf<double> J[2][2], D[2][2];   // [round parity][plane]: rotations J_P and transformed diagonal tiles; the lookahead
                                     // solve of round r+1 writes one parity while round r reads the other
  DevBuf<double> diag, scal;
  DevBuf<unsigned long long> off;    // one accumulator per sweep (ring)
  DevBuf<int> perm;
  DevBuf<unsigned int> work;         // one work counter per round (fused round kernel)
  GemmWorkspace lr_gws;              // Cholesky LR step
  DevBuf<double> lr_R[2], lr_T[2];
  // hipEvent timing of the fused round launches (one event pair around the rounds of each sweep, read at the sweep's
  // own host synchronisation): what bench.py's roofline of jacobi_fused_round_kernel is computed from
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  double round_ms = 0.0;
  long long round_launches = 0;
  GemmWorkspace gws;             // products of the tridiagonal route's back-transformation and clean-up
  TrdWorkspace trd;              // tridiagonal route (tridiag.h)
  TrdVecWorkspace trdv;          // ... its eigenvectors (tridiag_vec.h)
  DevBuf<double> lam_tmp;
  ~EvdWorkspace() {
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
  }
};

constexpr int JAC_OFF_RING = 64;

// The block Jacobi sweeps:  A = U diag(lam) U^H, lam descending.
//   Ar/Ai : n x n row-major planes (Ai == nullptr for a real symmetric matrix), lda
//   lam_host : n eigenvalues (descending); lam_dev (nullable) gets the same on the device
//   Zr/Zi : n x n, row i = conj(u_i)   (ldz); Zr == nullptr: eigenvalues only
//   tol : stop when the largest off-diagonal entry a sweep leaves behind is below tol * scale
template <bool CPLX, int NT>
void jacobi_evd(hipStream_t st, EvdWorkspace& ws, const double* Ar, const double* Ai, int n, int64_t lda,
                std::vector<double>& lam_host, double* lam_dev, double* Zr, double* Zi, int64_t ldz, const double tol,
                EvdInfo* info) {
  int max_sweeps = 50;
  if (const char* e = std::getenv("XMCA_JACOBI_MAX_SWEEPS")) { if (std::atoi(e) > 0) max_sweeps = std::atoi(e); }   // (tests: the non-convergence error)
  if (info) *info = EvdInfo{};
  const int S = std::max(ceil_div(n, NT), 1);
  const int npad = S * NT;
  const size_t nn = (size_t)npad * npad;
  const bool want_z = Zr != nullptr;      // eigenvalues only: the eigenvector tiles (half of the work) are skipped
  for (int b = 0; b < 2; ++b) {
    ws.G[b][0].ensure(nn);
    if (want_z) ws.Z[b][0].ensure(nn);
    ws.J[b][0].ensure((size_t)S * NT * NT);
    ws.D[b][0].ensure((size_t)S * NT * NT);
    if (CPLX) {
      ws.G[b][1].ensure(nn);
      if (want_z) ws.Z[b][1].ensure(nn);
      ws.J[b][1].ensure((size_t)S * NT * NT);
      ws.D[b][1].ensure((size_t)S * NT * NT);
    }
  }
  ws.diag.ensure((size_t)npad);
  ws.scal.ensure(8);
  ws.off.ensure(JAC_OFF_RING);
  ws.perm.ensure((size_t)npad);
  if (max_sweeps > JAC_OFF_RING - 2) max_sweeps = JAC_OFF_RING - 2;   // the last slot holds the post-sweep measure

  XMCA_HIP(hipMemsetAsync(ws.off.get(), 0, sizeof(unsigned long long) * JAC_OFF_RING, st));
  XMCA_HIP(hipMemsetAsync(ws.scal.get(), 0, sizeof(double) * 8, st));
  if (npad > n)
    hipLaunchKernelGGL(jacobi_frobenius_kernel, dim3(std::min(n, 1024)), dim3(256), 0, st, Ar, CPLX ? Ai : nullptr, n, lda, ws.scal.get());
  hipLaunchKernelGGL(jacobi_init_scale_kernel, dim3(1), dim3(256), 0, st, Ar, n, lda, 1e-13, ws.scal.get());
  hipLaunchKernelGGL(jacobi_init_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, Ar, CPLX ? Ai : nullptr, n, lda,
                     ws.G[0][0].get(), CPLX ? ws.G[0][1].get() : nullptr, want_z ? ws.Z[0][0].get() : nullptr,
                     (CPLX && want_z) ? ws.Z[0][1].get() : nullptr, npad, ws.scal.get());
  XMCA_HIP(hipGetLastError());

  const double tile_tol = 2e-15;
  const bool lookahead = S >= 3;       // (the fused round with the look-ahead tile solves; the unfused form was slower)

  int cur = 0;
  const int rounds = (S == 1) ? 1 : 2 * S - 1;
  const int zchunks = want_z ? (S + JAC_ZW - 1) / JAC_ZW : 0;   // 0: the launches simply do not contain Z tiles
  const int n_off = S * (S - 1) / 2;
  // Inexact inner solves: a diagonal tile is swept only ONCE per visit.  Measured on MI355X (C2, T = 2920): 1 sweep per
  // visit needs the same 13 outer sweeps as a full tile solve at a third of the time; more were measured slower overall.
  // Tiles are swept in full once per outer sweep (its first round), cross-block only otherwise.
  auto is_cross = [&](int round_in_sweep) { return S > 1 && round_in_sweep != 0; };
  auto evd = [&](hipStream_t s, int gbuf, int par, int sweep_slot, int round_in_sweep) {
    hipLaunchKernelGGL((jacobi_tile_evd_kernel<NT, CPLX>), dim3(S), dim3(jac_threads<NT>()), 0, s, ws.G[gbuf][0].get(),
                       CPLX ? ws.G[gbuf][1].get() : nullptr, npad, ws.J[par][0].get(), CPLX ? ws.J[par][1].get() : nullptr,
                       ws.D[par][0].get(), CPLX ? ws.D[par][1].get() : nullptr, tile_tol, ws.scal.get(),
                       ws.off.get() + sweep_slot, S == 1 ? 60 : 1, is_cross(round_in_sweep) ? 1 : 0);
  };
  auto update = [&](hipStream_t s, int par, int grid) {
    hipLaunchKernelGGL((jacobi_update_kernel<NT, CPLX>), dim3(grid), dim3(jac_threads<NT>()), 0, s, ws.G[cur][0].get(),
                       CPLX ? ws.G[cur][1].get() : nullptr, ws.G[cur ^ 1][0].get(), CPLX ? ws.G[cur ^ 1][1].get() : nullptr,
                       ws.Z[cur][0].get(), CPLX ? ws.Z[cur][1].get() : nullptr, ws.Z[cur ^ 1][0].get(),
                       CPLX ? ws.Z[cur ^ 1][1].get() : nullptr, ws.J[par][0].get(), CPLX ? ws.J[par][1].get() : nullptr,
                       ws.D[par][0].get(), CPLX ? ws.D[par][1].get() : nullptr, S, npad);
  };

  // fused rounds: persistent workgroups (two per CU) pull items from one counter per round
  const int zch2 = want_z ? S : 0;
  const int fused_items = n_off + S * zch2;
  static const int resident_wgs = [] {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return jacobi_fused_wgs_per_cu<NT>() * cus;
  }();
  const int fused_grid = std::max(S, std::min(resident_wgs, S + fused_items));
  const int n_workers = fused_grid - S;
  // eigenvector tiles handed out statically per worker (the G tiles always are): the whole even split (a sweep of the
  // share, 75..100 %, was flat above 90 %: profiles/r02_*)
  const int n_static = n_workers <= 0 ? 0 : S * zch2 / n_workers;
  // eigenvalues only: the tile solves get their CUs to themselves
  // (measured: eigenvalues of a 2920^2 real matrix 57.5 -> 51.8 ms; with four workgroups per CU - the 32 x 32 complex
  //  tiles - a quarter of the workers would leave and the solve gets slower, 86 -> 95 ms at n = 2501)
  const int ncu = resident_wgs / jacobi_fused_wgs_per_cu<NT>();
  const bool exile = !want_z && jacobi_fused_wgs_per_cu<NT>() == 2 && fused_grid == resident_wgs && S < ncu / 2;
  const int exile_ncu = exile ? ncu : 0;
  if (lookahead) {
    ws.work.ensure((size_t)max_sweeps * rounds);
    XMCA_HIP(hipMemsetAsync(ws.work.get(), 0, sizeof(unsigned int) * (size_t)max_sweeps * rounds, st));
  }

  int sweeps = 0;
  double off = 0.0;
  int64_t round_no = 0;
  bool lr_applied = false;
  bool converged = S == 1;      // (a single tile is solved to its own tolerance inside the kernel)
  double lr_delta = 0.0, last_left = 0.0;
  if (lookahead) evd(st, cur, 0, 0, 0);  // diagonal tiles of the very first round
  if (lookahead && !ws.ev_a) {
    XMCA_HIP(hipEventCreate(&ws.ev_a));
    XMCA_HIP(hipEventCreate(&ws.ev_b));
  }
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    if (lookahead) XMCA_HIP(hipEventRecord(ws.ev_a, st));
    for (int r = 0; r < rounds; ++r, ++round_no) {
      const int par = (int)(round_no & 1);
      if (!lookahead) {
        evd(st, cur, par, sweep, r);
        update(st, par, S + n_off + S * zchunks);
      } else {
        // ONE launch: tile solves of round r+1 (assembled from this round's G, J, D) + the whole update of round r.
        // Cross code 3 = cross-block sweep, in its two-level form where there is one (64 x 64 real tiles: 85k against the
        // flat sweep's 127k cycles per round); the 32 x 32 tiles take the flat cross sweep.
        const int next_slot = (r == rounds - 1) ? sweep + 1 : sweep;
        hipLaunchKernelGGL((jacobi_fused_round_kernel<NT, CPLX>), dim3(fused_grid), dim3(jac_threads<NT>()), 0, st,
                           ws.G[cur][0].get(), CPLX ? ws.G[cur][1].get() : nullptr, ws.G[cur ^ 1][0].get(),
                           CPLX ? ws.G[cur ^ 1][1].get() : nullptr, ws.Z[cur][0].get(), CPLX ? ws.Z[cur][1].get() : nullptr,
                           ws.Z[cur ^ 1][0].get(), CPLX ? ws.Z[cur ^ 1][1].get() : nullptr, ws.J[par][0].get(),
                           CPLX ? ws.J[par][1].get() : nullptr, ws.D[par][0].get(), CPLX ? ws.D[par][1].get() : nullptr,
                           ws.J[par ^ 1][0].get(), CPLX ? ws.J[par ^ 1][1].get() : nullptr, ws.D[par ^ 1][0].get(),
                           CPLX ? ws.D[par ^ 1][1].get() : nullptr, tile_tol, ws.scal.get(), ws.off.get() + next_slot,
                           1, is_cross((r + 1) % rounds) ? 3 : 0, S, npad, ws.work.get() + round_no, zch2, n_static,
                           exile_ncu);
      }
      cur ^= 1;
    }
    if (lookahead) XMCA_HIP(hipEventRecord(ws.ev_b, st));
    XMCA_HIP(hipGetLastError());
    // two measures per sweep: `off` = the largest entry the sweep met when it visited the tiles (also carries the NaN
    // flag), `left` = the largest entry of the matrix it leaves behind (one 25 us pass).  Stopping on `left` saves the
    // sweep that would only confirm convergence.
    unsigned long long bits[2] = {0, 0};
    if (S > 1) {
      XMCA_HIP(hipMemsetAsync(ws.off.get() + JAC_OFF_RING - 1, 0, sizeof(unsigned long long), st));
      if (lr_applied)
        hipLaunchKernelGGL(jacobi_diag_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, ws.G[cur][0].get(), npad, ws.diag.get());
      hipLaunchKernelGGL(jacobi_offmax_kernel, dim3(1024), dim3(256), 0, st, ws.G[cur][0].get(), CPLX ? ws.G[cur][1].get() : nullptr,
                         npad, NT / 2, ws.scal.get(), lr_applied ? ws.diag.get() : nullptr, ws.off.get() + JAC_OFF_RING - 1);
      XMCA_HIP(hipMemcpyAsync(&bits[1], ws.off.get() + JAC_OFF_RING - 1, sizeof(bits[1]), hipMemcpyDeviceToHost, st));
    }
    XMCA_HIP(hipMemcpyAsync(&bits[0], ws.off.get() + sweep, sizeof(bits[0]), hipMemcpyDeviceToHost, st));
    XMCA_HIP(hipStreamSynchronize(st));
    if (lookahead) {
      float t = 0.f;
      XMCA_HIP(hipEventElapsedTime(&t, ws.ev_a, ws.ev_b));
      ws.round_ms += t;
      ws.round_launches += rounds;
    }
    std::memcpy(&off, &bits[0], sizeof(double));
    double left = off;
    if (S > 1) std::memcpy(&left, &bits[1], sizeof(double));
    last_left = left;
    ++sweeps;
    static const bool trace = xmca_trace("jacobi");
    if (trace) std::fprintf(stderr, "[xmca jacobi f64] n=%d NT=%d cplx=%d sweep %d: max off/scale seen = %.3e, left = %.3e\n", n, NT, (int)CPLX, sweeps, off, left);
    if (S == 1) break;
    if (!(left >= tol) || !std::isfinite(left)) { off = left; converged = true; break; }   // (NaN is reported below)
    // Cholesky LR step for graded spectra.  With eigenvalues spread evenly over many decades the couplings between
    // large and small eigenvalues have to fall far below the small ones before those start to converge, and the
    // sweeps only converge linearly (measured: 30 sweeps for 12 decades at n = 2920, 12 for a flat bulk).  One step of
    // the Cholesky LR iteration, G + delta I = R^H R -> M = R R^H (= R G R^-1 + delta I), removes exactly these
    // long-range couplings (11 sweeps for the same matrix); it costs about one sweep, so it is taken only when the
    // diagonal after `lr_after` sweeps says the spectrum is graded.  Z <- R Z turns the accumulated rows into
    // sqrt(lambda_i) x eigenvector, which the final gather normalises.
    static const int lr_mode = [] { const char* e = std::getenv("XMCA_JACOBI_LR"); return e ? std::atoi(e) : 1; }();   // 0 off, 1 auto, 2 always
    constexpr double lr_spread = 100.0;     // q10 / q90 of the sorted diagonal beyond which the spectrum counts as graded
    constexpr int lr_after = 2;             // ... looked at after the second sweep
    if (lookahead && lr_mode != 0 && sweeps == lr_after && !lr_applied) {
      hipLaunchKernelGGL(jacobi_diag_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, ws.G[cur][0].get(), npad, ws.diag.get());
      std::vector<double> dd(npad);
      XMCA_HIP(hipMemcpyAsync(dd.data(), ws.diag.get(), sizeof(double) * npad, hipMemcpyDeviceToHost, st));
      XMCA_HIP(hipStreamSynchronize(st));
      std::vector<int> pm(npad);
      for (int i = 0; i < npad; ++i) pm[i] = i;
      std::stable_sort(pm.begin(), pm.end(), [&](int a, int b) { return dd[a] > dd[b]; });
      // the padding (-scale, decoupled) must be what sorts last; a matrix with diagonal entries down there is not a
      // Gram matrix and stays on the plain path
      const double dmax = dd[pm[0]], dmin = dd[pm[n - 1]];
      const double q10 = dd[pm[n / 10]], q90 = std::max(dd[pm[(int64_t)n * 9 / 10]], 1e-14 * dmax);
      const double spread = (dmax > 0.0 && q10 > 0.0) ? q10 / q90 : 0.0;
      if (info) info->diag_spread = spread;
      if (dmin > -0.25 * dmax && dmax > 0.0 && std::isfinite(dmax) && (lr_mode == 2 || spread > lr_spread)) {
        XMCA_HIP(hipMemcpyAsync(ws.perm.get(), pm.data(), sizeof(int) * npad, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(jacobi_permute_kernel, dim3(std::min(ceil_div(npad, 256), 16), npad), dim3(256), 0, st, ws.G[cur][0].get(),
                           CPLX ? ws.G[cur][1].get() : nullptr, want_z ? ws.Z[cur][0].get() : nullptr,
                           (CPLX && want_z) ? ws.Z[cur][1].get() : nullptr, npad, NT / 2, ws.perm.get(), ws.G[cur ^ 1][0].get(),
                           CPLX ? ws.G[cur ^ 1][1].get() : nullptr, want_z ? ws.Z[cur ^ 1][0].get() : nullptr,
                           (CPLX && want_z) ? ws.Z[cur ^ 1][1].get() : nullptr);
        XMCA_HIP(hipGetLastError());
        cur ^= 1;
        const size_t row = sizeof(double) * (size_t)n, pitch = sizeof(double) * (size_t)npad;
        for (int pl = 0; pl < (CPLX ? 2 : 1); ++pl) {
          ws.lr_R[pl].ensure((size_t)n * n);
          XMCA_HIP(hipMemcpy2DAsync(ws.lr_R[pl].get(), row, ws.G[cur][pl].get(), pitch, row, n, hipMemcpyDeviceToDevice, st));
        }
        double* Rr = ws.lr_R[0].get();
        double* Ri = CPLX ? ws.lr_R[1].get() : nullptr;
        const double rel_shift = 1e-13;
        if (cholesky_upper(st, ws.lr_gws, Rr, Ri, n, n, rel_shift)) {
          // M = R R^H over the leading block of G (the padding stays decoupled)
          cgemm<double>(st, ws.lr_gws, Rr, Ri, n, true, false, Rr, Ri, n, false, true, ws.G[cur][0].get(),
                        CPLX ? ws.G[cur][1].get() : nullptr, npad, n, n, n, 1.0, nullptr, nullptr, true);
          if (want_z) {
            for (int pl = 0; pl < (CPLX ? 2 : 1); ++pl) ws.lr_T[pl].ensure((size_t)n * n);
            cgemm<double>(st, ws.lr_gws, Rr, Ri, n, true, false, ws.Z[cur][0].get(), CPLX ? ws.Z[cur][1].get() : nullptr, npad, true, false,
                          ws.lr_T[0].get(), CPLX ? ws.lr_T[1].get() : nullptr, n, n, n, n, 1.0, nullptr, nullptr, false);
            for (int pl = 0; pl < (CPLX ? 2 : 1); ++pl)
              XMCA_HIP(hipMemcpy2DAsync(ws.Z[cur][pl].get(), pitch, ws.lr_T[pl].get(), row, row, n, hipMemcpyDeviceToDevice, st));
          }
          lr_applied = true;
          lr_delta = rel_shift * dmax;
          // M is positive definite with a meaningful (graded) diagonal: from here on rotations and the stopping rule are
          // relative to sqrt(m_ii m_jj) alone - the orthogonality of the back-transformed vectors is the scaled
          // off-diagonal part of the final M - and the absolute rotation floor is dropped
          XMCA_HIP(hipMemsetAsync(ws.scal.get() + 1, 0, sizeof(double), st));
        }
        XMCA_HIP(hipStreamSynchronize(st));   // pm goes out of scope
        evd(st, cur, (int)(round_no & 1), sweep + 1, 0);   // the lookahead solve of the next round saw the old matrix
        if (trace) std::fprintf(stderr, "[xmca jacobi] n=%d diagonal spread q10/q90 = %.3e: Cholesky LR step %s\n", n, spread, lr_applied ? "taken" : "failed (not positive definite)");
      } else if (trace) {
        std::fprintf(stderr, "[xmca jacobi] n=%d diagonal spread q10/q90 = %.3e: no LR step\n", n, spread);
      }
    }
  }
  XMCA_CHECK(std::isfinite(off), XMCA_ERR_NUMERIC, "SVD failed. NaN entries may be the problem.");
  // like LAPACK's gesdd the solver either converges or says so: an unconverged basis is never returned as singular vectors
  if (!converged) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "SVD did not converge: %d Jacobi sweeps left relative off-diagonal entries of %.3e behind (limit %.1e)",
                  sweeps, last_left, tol);
    throw Error(XMCA_ERR_NUMERIC, msg);
  }

  // eigenvalues = diagonal; sort descending on the host, drop the padding (= the most negative entries)
  hipLaunchKernelGGL(jacobi_diag_kernel, dim3(ceil_div(npad, 256)), dim3(256), 0, st, ws.G[cur][0].get(), npad, ws.diag.get());
  std::vector<double> d(npad);
  XMCA_HIP(hipMemcpyAsync(d.data(), ws.diag.get(), sizeof(double) * npad, hipMemcpyDeviceToHost, st));
  XMCA_HIP(hipStreamSynchronize(st));
  std::vector<int> perm(npad);
  for (int i = 0; i < npad; ++i) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return d[a] > d[b]; });
  lam_host.resize(n);
  for (int i = 0; i < n; ++i) lam_host[i] = d[perm[i]] - lr_delta;
  XMCA_HIP(hipMemcpyAsync(ws.perm.get(), perm.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
  if (lam_dev) XMCA_HIP(hipMemcpyAsync(lam_dev, lam_host.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
  if (Zr && lr_applied) {
    hipLaunchKernelGGL(jacobi_gather_normalize_kernel, dim3(n), dim3(256), 0, st, ws.Z[cur][0].get(), CPLX ? ws.Z[cur][1].get() : nullptr,
                       npad, ws.perm.get(), n, Zr, CPLX ? Zi : nullptr, ldz);
    XMCA_HIP(hipGetLastError());
  } else if (Zr) {
    hipLaunchKernelGGL(jacobi_gather_kernel, dim3(std::min(ceil_div(n, 256), 64), n), dim3(256), 0, st, ws.Z[cur][0].get(),
                       CPLX ? ws.Z[cur][1].get() : nullptr, npad, ws.perm.get(), n, Zr, CPLX ? Zi : nullptr, ldz);
    XMCA_HIP(hipGetLastError());
  }
  XMCA_HIP(hipStreamSynchronize(st));   // perm / lam_host staging buffers go out of scope
  if (info) { info->sweeps = sweeps; info->tile = NT; info->slots = S; info->last_off = off; info->lr_step = lr_applied ? 1 : 0; info->n_eigvec = Zr ? n : 0; }
}

// Hermitian EVD  A = U diag(lam) U^H, lam descending (see jacobi_evd for the arguments).
//
// Two solvers share this entry point: the reduction to tridiagonal form (tridiag.h, tridiag_vec.h: eigenproblems of 192 and
// more without vectors, 768 and more with vectors) and the block Jacobi sweeps of this file (everything else, nearly
// diagonal problems, and spectra with clusters the tridiagonal route hands back).
// The guard of the partial route.  lam: all n eigenvalues, descending.  Returns the first k' >= n_lead behind which the spectrum
// is clear of the computed set - or n when no such k' lies within the cap (the caller then forms all vectors).  DESIGN.md 2.10:
//   * twisted vectors of lam_k', lam_k'+1 overlap by up to eps ||T|| / (lam_k' - lam_k'+1) (tridiag_vec.h); inside the set the
//     clean-up repairs an overlap up to 0.3, across the cut nothing can.  What the cut may leave behind is held to what one
//     Newton-Schulz step leaves of the largest defect the clean-up accepts, (3/4) 0.3^2;
//   * a pair that agrees to a relative gap below 1e-3 - the bound below which the MRRR literature (LAPACK dlarrv, MINRGP) stops
//     trusting independent twisted vectors, eps / relgap ~ 2e-13, the square of the 1e-6 at which the clean-up is one step from
//     done - is a cluster as far as the vectors are concerned and is kept whole.
constexpr double TRD_PARTIAL_RELGAP = 1e-3;
constexpr double TRD_PARTIAL_LEAK = 0.75 * 0.3 * 0.3;
constexpr int TRD_PARTIAL_CAP = 32;            // half a block of the twisted kernel
inline int trd_partial_count(const std::vector<double>& lam, int n, int n_lead) {
  if (n_lead < 1 || n_lead >= n) return n;
  const double norm = std::max(std::fabs(lam.front()), std::fabs(lam.back()));
  const int last = std::min(n_lead + TRD_PARTIAL_CAP, n - 1);
  for (int k = n_lead; k <= last; ++k) {       // k vectors: the cut lies between lam[k-1] and lam[k]
    const double gap = lam[(size_t)k - 1] - lam[(size_t)k];
    const bool rel_ok = gap > TRD_PARTIAL_RELGAP * std::fabs(lam[(size_t)k - 1]);
    const bool abs_ok = 2.220446049250313e-16 * norm <= TRD_PARTIAL_LEAK * gap;
    if (rel_ok && abs_ok) return 4 * k <= n ? k : n;      // (a set of more than n / 4 vectors is no longer thin)
  }
  return n;
}

// The `repeated` test of the partial route: bit-equal eigenvalues (to the last bit of the largest one in magnitude) among the
// leading kp + 1 - the set and its neighbour - go to the Jacobi sweeps, as on the full route.  lam: all n, descending.
inline bool trd_repeated_leading(const std::vector<double>& lam, int n, int kp) {
  const double lmax = n > 0 ? std::max(std::fabs(lam.front()), std::fabs(lam.back())) : 0.0;
  for (int i = 0; i < kp && i + 1 < n; ++i)
    if (lam[(size_t)i] - lam[(size_t)i + 1] <= 2.2e-16 * lmax) return true;
  return false;
}

// Which solver forms eigenvectors of a matrix of order n: the tridiagonal route (true) or the block Jacobi sweeps, which form all
// n vectors whatever is asked for.  XMCA_TRIDIAG_VEC_MIN_N (default 768), XMCA_TRIDIAG=0 and the route's size limits decide.
inline bool evd_vectors_by_reduction(int n, bool cplx) {
  const int trd_vec_min_n = [] { const char* e = std::getenv("XMCA_TRIDIAG_VEC_MIN_N"); return e ? std::atoi(e) : 768; }();
  return trd_enabled() && n >= trd_vec_min_n && trd_fits(n, cplx);
}

// n_lead: the number of leading eigenvectors wanted (Zr then needs n_lead rows only); < 0 or >= n: all of them, exactly the
// path of a call without the argument.  On the tridiagonal route fewer vectors than n are then FORMED as well (k' >= n_lead of
// them, info->n_eigvec: trd_partial_count, trd_eigenvectors_partial); where that route does not apply or the partial stage hands
// the problem back, all n are formed - from the same reduction - in scratch planes and the leading n_lead rows copied out.
// lead_hook (all vectors wanted, real): see TrdLeadHook - trd_eigenvectors fills it in its common case, nobody else touches it.
inline void hermitian_evd(hipStream_t st, EvdWorkspace& ws, const double* Ar, const double* Ai, int n, int64_t lda,
                          std::vector<double>& lam_host, double* lam_dev, double* Zr, double* Zi, int64_t ldz,
                          EvdInfo* info = nullptr, bool nearly_diagonal = false, int n_lead = -1, TrdLeadHook* lead_hook = nullptr) {
  const bool cplx = Ai != nullptr;
  const bool part = Zr && n_lead >= 0 && n_lead < n;
  if (part) XMCA_CHECK(n_lead >= 1, XMCA_ERR_INVALID, "hermitian_evd: n_lead must be at least 1 when vectors are wanted");
  // Where all n vectors have to be formed although the caller wants (and has room for) n_lead rows only, they go to scratch
  // planes of this call and the leading rows are copied out; the stream is synchronised before the planes are given back.
  DevBuf<double> full[2];
  double *Fr = Zr, *Fi = Zi;
  int64_t ldf = ldz;
  auto all_rows = [&] {
    if (!part || Fr != Zr) return;
    Fr = full[0].ensure((size_t)n * n);
    Fi = cplx ? full[1].ensure((size_t)n * n) : nullptr;
    ldf = n;
  };
  auto hand_out = [&] {
    if (!part) return;
    const size_t row = sizeof(double) * (size_t)n;
    XMCA_HIP(hipMemcpy2DAsync(Zr, sizeof(double) * (size_t)ldz, Fr, row, row, (size_t)n_lead, hipMemcpyDeviceToDevice, st));
    if (cplx) XMCA_HIP(hipMemcpy2DAsync(Zi, sizeof(double) * (size_t)ldz, Fi, row, row, (size_t)n_lead, hipMemcpyDeviceToDevice, st));
    XMCA_HIP(hipStreamSynchronize(st));
  };
  // `nearly_diagonal`: the caller knows that a few Jacobi sweeps finish the problem (the weak block of solver.h, three
  // sweeps) - cheaper than any reduction, whose cost does not depend on the matrix.
  // eigenvalues only (rule_n without rotation, every n_vec = 0 solve): Householder tridiagonalisation + Sturm multisection
  // (tridiag.h) - (4/3) n^3 flop in n launches instead of ~11 sweeps of 4 n^3.  XMCA_TRIDIAG=0 keeps the Jacobi sweeps.
  const int trd_min_n = [] { const char* e = std::getenv("XMCA_TRIDIAG_MIN_N"); return e ? std::atoi(e) : 192; }();
  if (!Zr && !nearly_diagonal && trd_enabled() && n >= trd_min_n && trd_fits(n, Ai != nullptr)) {
    TrdParams P = trd_reduce(st, ws.trd, Ar, Ai, n, lda, false);
    if (xmca_trace("trdsum")) trd_trace_checksums(st, P, Ar, n, lda);
    trd_eigenvalues(st, ws.trd, P, lam_host, lam_dev, ws.lam_tmp);
    if (info) {
      *info = EvdInfo{};
      info->tridiag = 1;
    }
    return;
  }
  // with eigenvectors: the same reduction, twisted-factorisation vectors of the tridiagonal matrix, back-transformation by
  // blocked reflectors and a Newton-Schulz clean-up (tridiag_vec.h).  Spectra with clusters the clean-up cannot repair
  // (repeated eigenvalues, null spaces of dimension > 1) come back here and take the Jacobi sweeps below.
  if (Zr && !nearly_diagonal && evd_vectors_by_reduction(n, Ai != nullptr)) {
    ws.trdv.count_call();
    TrdParams P = trd_reduce(st, ws.trd, Ar, Ai, n, lda, true);
    // The Sturm kernel is queued FIRST, so that it starts when the reduction ends and not behind the host's queueing of the
    // compact-WY launches; those wait for the reduction alone (the fork is recorded in front of the Sturm kernel) and run on
    // a second stream from the second call on, under the Sturm and twisted kernels - otherwise on `st` behind the Sturm kernel.
    trd_wy_fork(st, ws.trdv, P);
    std::vector<double> lam_t;
    trd_eigenvalues_launch(st, ws.trd, P, lam_dev, ws.lam_tmp, ws.trdv.lam_asc.ensure((size_t)n));
    trd_wy_prepare(st, ws.trdv, ws.gws, P, Ai != nullptr);
    trd_eigenvalues_collect(st, ws.trd, P, lam_t, ws.lam_tmp);
    if (part) {
      // The leading n_lead vectors only: k' of them are formed (the guard above).  Whatever keeps the partial stage from
      // finishing - no gap within the cap, more than n / 4 vectors, bit-equal leading values, a refused clean-up - goes on
      // below with THIS reduction and these eigenvalues: all vectors by the full stage, or the sweeps.
      const int kp = trd_partial_count(lam_t, n, n_lead);
      bool ran = false, done = false;
      // bit-equal eigenvalues among the leading k' + 1 (the set and its neighbour) go to the sweeps, as on the full route
      const bool rep_lead = trd_repeated_leading(lam_t, n, kp);
      if (kp < n && !rep_lead) {
        ran = true;
        done = trd_eigenvectors_partial(st, ws.trdv, ws.gws, P, cplx, kp, n_lead, Zr, Zi, ldz);
      }
      if (xmca_trace("solve"))
        std::fprintf(stderr, "xmca: eigh n = %d, %d leading vectors wanted: %d formed%s\n", n, n_lead, done ? kp : n,
                     done ? "" : (kp >= n ? " (no gap within the cap)" : rep_lead ? " (repeated eigenvalues)" : " (clean-up refused)"));
      if (done) {
        XMCA_HIP(hipStreamSynchronize(st));
        lam_host = lam_t;
        if (info) {
          *info = EvdInfo{};
          info->tridiag = 1;
          info->n_eigvec = kp;
        }
        return;
      }
      if (ran) ws.trdv.prepared = true;      // (joined by the partial stage; T V^H of every super-block is untouched)
    }
    // Eigenvalues that coincide to the last bit of the largest one (a null space of dimension > 1: repeated samples, low-rank
    // fields) are not resolved by the twisted vectors - the clean-up would find that out only after the back-transformation
    // and two n^3 products (advisor, round 3); they are on the host already, so the sweeps below start right away.
    bool repeated = false;
    {
      const double lmax = n > 0 ? std::max(std::fabs(lam_t.front()), std::fabs(lam_t.back())) : 0.0;
      for (int i = 0; i + 1 < n && !repeated; ++i) repeated = lam_t[(size_t)i] - lam_t[(size_t)i + 1] <= 2.2e-16 * lmax;
      if (repeated && xmca_trace("solve")) std::fprintf(stderr, "xmca: eigh n = %d: repeated eigenvalues - block Jacobi instead of twisted vectors\n", n);
    }
    if (repeated) {
      // The compact-WY factors queued above are not going to be used: wait for them here (second stream) so that they do not
      // run beside the Jacobi rounds, and leave the workspace as if nothing had been prepared (advisor, round 4).
      if (ws.trdv.prepared && !ws.trdv.joined && ws.trdv.side) XMCA_HIP(hipStreamSynchronize(ws.trdv.side));
      ws.trdv.prepared = false;
      ws.trdv.joined = true;
    }
    if (!repeated) all_rows();
    if (!repeated && trd_eigenvectors(st, ws.trd, ws.trdv, ws.gws, P, Ai != nullptr, Fr, Fi, ldf, part ? nullptr : lead_hook)) {
      XMCA_HIP(hipStreamSynchronize(st));
      lam_host = lam_t;
      if (info) {
        *info = EvdInfo{};
        info->tridiag = 1;
        info->n_eigvec = n;
      }
      hand_out();
      return;
    }
  }
  // stop after the first sweep that leaves no off-diagonal entry above 1e-10 * max|diag| behind: with the (at least
  // fast-linear, normally quadratic) convergence the next sweep would only confirm it
  // eigenvalues only (rule_n): an eigenvalue is off by sum_j |g_ij|^2 / (lam_i - lam_j), second order in what is left -
  // 1e-8 left behind bounds that by ~n 1e-16 lam_max for a spectrum without exact clusters, and the sweep that would
  // push the vectors' first-order error down is not needed (C4 surrogates: 12 -> 11 sweeps)
  const double tol = Zr ? 1e-10 : 1e-8;
  // tile size by problem kind (64 x 64 complex tiles do not fit the LDS of the update kernel)
  all_rows();
  if (Ai) jacobi_evd<true, 32>(st, ws, Ar, Ai, n, lda, lam_host, lam_dev, Fr, Fi, ldf, tol, info);
  else if (n > 32) jacobi_evd<false, 64>(st, ws, Ar, nullptr, n, lda, lam_host, lam_dev, Fr, nullptr, ldf, tol, info);
  else jacobi_evd<false, 32>(st, ws, Ar, nullptr, n, lda, lam_host, lam_dev, Fr, nullptr, ldf, tol, info);
  hand_out();
}

}  // namespace xmca
