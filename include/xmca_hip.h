/*
 * xmca_hip.h - C ABI of the MI355X (gfx950) implementation of the xmca solve / rotate / rule_n path.
 *
 * The reference (nicrie/xmca v1.4.2) is pure Python: it has no FFI of its own.  The drop-in boundary is
 * therefore the private numerical core of xmca.array.MCA, and every entry point below names the reference
 * lines it replaces.  The host side (xmca_amd/array.py) binds these symbols through ctypes; INTEGRATION.md
 * shows the stub a maintainer of the reference would add.  xmca_fill_gaps (DINEOF gap filling) stands beside
 * the model: it takes a field with NaN gaps and needs no resident state.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Return value: 0 = ok, negative = error code below;
 *     xmca_last_error() returns the message of the last failure on that handle.
 *   - The caller owns every host buffer.  The library owns all device memory inside the opaque handle.
 *   - One handle = one HIP device + one stream.  A handle is not thread-safe; use one per thread / rank.
 *   - Matrices are row-major.  Complex data is interleaved (re, im) in host buffers.
 *   - dtype: 0 = float32, 1 = float64 (of the real components).
 */
#ifndef XMCA_HIP_H
#define XMCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMCA_OK 0
#define XMCA_ERR_INVALID (-1)        /* bad argument                                   -> ValueError            */
#define XMCA_ERR_HIP (-2)            /* HIP runtime failure                            -> RuntimeError          */
#define XMCA_ERR_NOT_CONVERGED (-3)  /* Varimax hit max_iter (rotation.py:66-71)       -> RuntimeError          */
#define XMCA_ERR_STATE (-4)          /* call order (e.g. vectors before solve)         -> RuntimeError          */
#define XMCA_ERR_UNSUPPORTED (-5)    /* outside device limits                          -> NotImplementedError   */
#define XMCA_ERR_NUMERIC (-6)        /* NaN / singular matrix (array.py:575-578)       -> numpy LinAlgError     */

#define XMCA_F32 0
#define XMCA_F64 1
#define XMCA_HOST 0
#define XMCA_DEVICE 1

typedef struct xmca_handle xmca_handle;

/* library / device management ------------------------------------------------------------------------- */
const char* xmca_version(void);
/* Number of this header's ABI (XMCA_ABI_VERSION): the binding refuses a library built from another revision. */
#define XMCA_ABI_VERSION 16
int xmca_abi_version(void);
int xmca_device_count(void);
int xmca_create(int device, xmca_handle** out);
void xmca_destroy(xmca_handle* h);
const char* xmca_last_error(xmca_handle* h);

/* Input of solve(): the centered, weighted, NaN-free T x N field of one side (0 = left, 1 = right), i.e.
 * MCA._fields[key] as returned by MCA._get_X()                         (xmca/array.py:95, :117, :289-298).
 *   re        real part, T*N elements of `dtype`
 *   im        imaginary part (analytic signal computed by the host, array.py:455-470) or NULL
 *   location  XMCA_HOST: copied to the device;  XMCA_DEVICE: device pointers, adopted without a copy
 *             (they must stay valid until the next xmca_set_field / xmca_destroy). */
int xmca_set_field(xmca_handle* h, int side, const void* re, const void* im, int64_t T, int64_t N, int dtype, int location);

/* xmca_set_field for a real field that already lives on the handle's GPU, in any two-stride layout (an entry point added to ABI 15 -
 * no existing signature changes): element (t, n) of the T x N field is re[t * stride_t + n * stride_n], strides in elements, not
 * negative.  The field is COPIED into the library's own buffer as a contiguous row-major T x N array, so xmca_compact_field,
 * xmca_center_field, xmca_scale_field and the solve work as after a host upload; the caller's memory is never written and is not
 * referenced after the call returns (the handle's stream is synchronised).  Checks and state changes are those of xmca_set_field.
 * The copy kernel is chosen from the strides (xmca_ingest_regime): XMCA_INGEST_ROWS for stride_n == 1 - contiguous rows stride_t
 * apart, moved 16 bytes per lane where source and destination row are both 16-byte aligned, element by element otherwise (a column
 * slice of a wider array);  XMCA_INGEST_TRANSPOSE for stride_t == 1 - time is the fast axis, as in a (space, time) array handed
 * over transposed: 64 x 64 tiles through LDS, both sides coalesced;  XMCA_INGEST_GATHER for anything else (steps along both
 * axes).  A dimension of one element counts as contiguous.  The caller orders its own work on `re` before the call. */
#define XMCA_INGEST_ROWS 0
#define XMCA_INGEST_TRANSPOSE 1
#define XMCA_INGEST_GATHER 2
int xmca_set_field_strided(xmca_handle* h, int side, const void* re, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype);
/* The regime xmca_set_field_strided takes for a T x N view (no handle, no device); XMCA_ERR_INVALID for a negative stride or an
 * empty view. */
int xmca_ingest_regime(int64_t T, int64_t N, int64_t stride_t, int64_t stride_n);

/* Hilbert complexify on the device: X_im = Ht * X_re for every field set so far.  Ht (T x T) is the imaginary
 * part of the analytic-signal operator, imag(scipy.signal.hilbert(eye(T), axis=0)); it is circulant, so the
 * caller passes only its first column `hilbert_col` (T float64, host): Ht[t][s] = hilbert_col[(t - s) mod T].
 * Replaces scipy.signal.hilbert(field, axis=0) of array.py:464 for extend=False.
 * hilbert_col == NULL reverts to the real fields (a later solve on the same resident fields is a real one again). */
int xmca_complexify(xmca_handle* h, const double* hilbert_col);

/* Complexify with the fore/back-cast extension of solve(complexify=True, extend='exp', period=theta) on the device (ABI 10).
 * Replaces the host path of xmca/array.py:378-472 (`_get_reg_coefs`, `_exp_forecast`, `_extend`, `_complexify`: regression and
 * exponential forecast of every column, the 3T-long series, scipy.signal.hilbert, the trim to [T, 2T) and `remove_mean`).  For
 * extend='exp' that procedure is one linear operator along time, the same for every column: X~ = X + i G X with
 *   G[t][s] = col3[(t - s) mod 3T] - hbar[s] + sum_{k < rank} U[t][k] W[s][k]
 * (xmca_amd/_hip.py extended_imag_parts derives it).  col3: 3T float64, the first column of the imaginary Hilbert
 * operator at length 3T; hbar: T float64, the column means of its middle block; U, W: T x rank row-major float64 (rank <= 16).
 * All host memory, O(T); the T x T operator is assembled on the device and X_im = G X formed by the solve (never the
 * subspace formulation of xmca_complexify, which is exact for the circulant operator only) or by xmca_project.
 * Float32 fields are promoted to float64 on the device first, as the reference extends in float64: the resident fields are
 * float64 from then on (xmca_get_field returns float64; xmca_scale_field takes float64 factors).
 * Undone by xmca_complexify(h, NULL) or the next xmca_set_field of the left field, like xmca_complexify. */
int xmca_complexify_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W, int rank);

/* Complexify with the Theta fore/back-cast of solve(complexify=True, extend='theta', period=m) on the device (an entry point added to
 * ABI 15 - no existing signature changes).  Replaces the host path of xmca/array.py:367-376, :429-472 (one statsmodels ThetaModel
 * per grid point, forecast and backcast).  The extension is the one DESIGN.md 2.11 defines: additive seasonal means from the centred
 * moving average of length m, the least-squares drift b0 of the deseasonalised column, simple exponential smoothing with alpha on
 * [1e-4, 1 - 1e-4] found by six rounds of 33 grid candidates, and the forecast
 *   f_h = 0.95 b0 (h + (1 - (1 - alpha)^T) / alpha) + level + s[(T + h) mod m],   h = 0 .. T-1;
 * the backcast is the same map of the reversed column, reversed.  The fit is not linear in the column, its forecast is linear in
 * 2 + m fitted coefficients c = (level + 0.95 b0 (1 - (1 - alpha)^T) / alpha, 0.95 b0, s_0 .. s_{m-1}), so
 *   X_im = G0 X + B C,   G0[t][s] = col3[(t - s) mod 3T] - hbar[s]
 * with G0 the operator of xmca_complexify_extended at rank 0 and C (2 (2 + m) x N) the coefficients of every column, fitted by
 * the kernels of csrc/theta.h and never leaving the device.
 *   col3, hbar  as in xmca_complexify_extended
 *   B           T x 2 (2 + m) row-major float64, host memory: the images under the 3T Hilbert operator (rows [T, 2T), column means
 *               removed) of the forecast basis (1, h, the m indicators of (T + h) mod m) placed at [2T, 3T), then of the backcast
 *               basis (the same columns in reversed time) placed at [0, T)     (xmca_amd/_hip.py theta_imag_parts)
 *   period      m >= 1 with T >= 2 m; XMCA_ERR_INVALID otherwise
 * Float32 fields are promoted to float64 first, as by xmca_complexify_extended.  Undone by xmca_complexify(h, NULL) or the next
 * xmca_set_field of the left field. */
int xmca_complexify_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period);

/* The Theta fits behind xmca_complexify_theta of the resident real field of `side`, to host memory (parity tests; an entry point
 * added to ABI 15).  out: 2 x (3 + m) x N float64, the forecast's fit and then the backcast's (the fit of the reversed column), each
 * the rows alpha, b0, level, s_0 .. s_{m-1} over the N columns.  A column's values are the same bits on every call.  The resident
 * fields are not changed (a float32 field is fitted through a float64 copy). */
int xmca_theta_fit(xmca_handle* h, int side, int period, double* out);

/* Imaginary plane of the resident float64 field of `side` after xmca_complexify_extended / xmca_complexify_theta (an entry point
 * added to ABI 15): out, T x N float64, host memory - with xmca_get_field the analytic signal the solve worked on.  The planes are
 * formed first when no solve or projection has done so; XMCA_ERR_STATE when the field has no imaginary plane. */
int xmca_get_field_imag(xmca_handle* h, int side, double* out);

/* MCA.solve numerical core (xmca/array.py:549-584): per-field SVD, kernel, kernel SVD, back-projection.
 *   n_fields  1 (EOF/PCA) or 2 (MCA)
 *   n_vec     number of leading modes to back-project into grid space; -1 = all `rank` modes
 *             (two float64 fields: the re-solve of weak modes - deflation / weak-block refinement, DESIGN.md 1 - covers the
 *             modes that get vectors; with 0 <= n_vec < rank the singular values beyond n_vec are those of the single solve,
 *             accurate to ~5e-14 (sigma_1 / sigma_i)^2 relative)
 *   rank_out  min(T, Nx, Ny)  (array.py:597)
 * A one-field solve may return with the back-projection of the modes >= 256 still in flight on a second stream of the handle;
 * every entry point that reads those modes, touches the fields or solves again waits for it first (and reports its failure),
 * so callers see complete results in any call order.  XMCA_DEFER_BACKPROJECT=0: everything is finished before xmca_solve returns. */
int xmca_solve(xmca_handle* h, int n_fields, int64_t n_vec, int64_t* rank_out);

/* MCA._singular_values (array.py:590): all `rank` singular values of A^H B / (T-1), descending, float64. */
int xmca_get_singular_values(xmca_handle* h, double* out, int64_t n);

/* MCA._V[key] (array.py:584), transposed: out[m * N + n] = V[n][m] for m < n_modes; complex interleaved when
 * the model is complex.  dtype selects float32 / float64 components. */
int xmca_get_vectors(xmca_handle* h, int side, void* out, int64_t n_modes, int dtype);

/* MCA.eofs() in its final layout (array.py:615-646 `_get_V` + :676-721 `_get_eofs`, ABI 9): out[n * q + c] = sum_{mm < m} V[n][mm] W[mm][c]
 * for the N grid points of `side` - the N x q array the reference reshapes to (space..., modes) - mixed on the device from the
 * resident mode-major vectors, so the host neither transposes nor multiplies an N x m array.  W (m x q, row-major float64,
 * complex interleaved when w_is_complex) = diag(sqrt(s)) R / norm with its columns ordered and selected by the caller; W == NULL:
 * the first q = m vectors as they are.  The output is complex (interleaved) when the model or W is; dtype: float32 / float64. */
int xmca_get_eofs(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, void* out, int dtype);

/* Spatial maps in their final layout: MCA.eofs() with a scaling, a phase shift or masked grid points, spatial_amplitude() and
 * spatial_phase() (xmca/array.py:690-712, :1090-1093, :1122; an entry point added to ABI 14 - no existing signature changes).  The
 * compact values z[n][c] = (sum_{mm < m} V[n][mm] W[mm][c]) * col_factor[c] of the N' grid points of `side` are those of xmca_get_eofs
 * (W, m, q, w_is_complex as there; W == NULL: the first q = m vectors), times a per-column factor.
 *   col_factor  q float64 values, interleaved complex when factor_is_complex, host memory (the 'eigen' norms, the phase shift
 *               e^{i phi}), or NULL
 *   keep_idx    N' increasing row indices (int64) below N_full: the grid points the model kept, as in xmca_correlation_maps; every other
 *               row of `out` is NaN (both planes of a complex output).  NULL: N_full = N', no masked points
 *   kind        XMCA_MAP_EOF: z, complex (interleaved) when the model, W or the factor is;  XMCA_MAP_AMPLITUDE: sqrt(re^2 + im^2), real;
 *               XMCA_MAP_PHASE: atan2(im, re), real (a real model has im = +0: 0 or pi)
 *   scaling     XMCA_SCALE_NONE;  XMCA_SCALE_MAX: column c is divided by its largest |Re z| (EOF) or amplitude (AMPLITUDE) over the N'
 *               points;  XMCA_SCALE_STD (EOF only): by the population standard deviation (ddof 0) of Re z.  Any other combination is
 *               XMCA_ERR_INVALID.  The division is plain IEEE: a zero column gives inf / NaN as numpy does
 *   out         N_full x q of `dtype` (XMCA_F32 / XMCA_F64 components), host memory
 *   stat_out    NULL, or q float64 divisors (written when scaling is not NONE)
 * The statistics are float64 sums merged in a fixed order (no atomics): two calls give the same bits.  With scaling NONE and no factor
 * the kept rows are bit for bit those of xmca_get_eofs.  The resident fields, vectors and rotation state are not changed. */
#define XMCA_MAP_EOF 0
#define XMCA_MAP_AMPLITUDE 1
#define XMCA_MAP_PHASE 2
#define XMCA_SCALE_NONE 0
#define XMCA_SCALE_MAX 1
#define XMCA_SCALE_STD 2
int xmca_get_maps(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, const double* col_factor,
                  int factor_is_complex, const int64_t* keep_idx, int64_t N_full, int kind, int scaling, void* out, int dtype,
                  double* stat_out);

/* xmca_get_maps with the memory space of `out` as an argument (an entry point added to ABI 15 - no existing signature changes).
 *   out_location  XMCA_HOST: xmca_get_maps, to the bit.  XMCA_DEVICE: `out` is memory of the handle's GPU holding N_full x q
 *                 values of `dtype` (interleaved complex as above - torch's complex layout); the finishing kernel writes it
 *                 directly, nothing crosses to the host.  stat_out stays host memory.
 * The handle's stream is synchronised before the call returns; the caller orders its own work on `out` before the call. */
int xmca_get_maps_to(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, const double* col_factor,
                     int factor_is_complex, const int64_t* keep_idx, int64_t N_full, int kind, int scaling, void* out, int dtype,
                     double* stat_out, int out_location);

/* PC projection of MCA._get_U (xmca/array.py:648-674, the product `fields[k] @ V[k]`): U = X~ V with X~ the field of
 * `side` as solve() saw it - still resident on the device; the analytic signal X + i Ht X when complexify was
 * requested (the imaginary field plane is not needed: U = W + i Ht W with W = X V); X + i G X after
 * xmca_complexify_extended (the imaginary planes G X are formed first when the solve has not done so).
 *   V      N x m row-major, float64 (is_complex = 0) or interleaved complex128 (is_complex = 1), host memory
 *   U_out  T x m row-major float64, interleaved complex128 when *out_is_complex = 1 (model or V complex)
 *   V == NULL (ABI 11): the first m vectors of the last solve, still resident on the device (N = their length, m <= the modes
 *          back-projected); is_complex is then ignored
 * The scaling by 1/sqrt(sigma) and the rotation (array.py:391-393) stay with the caller (m x m work). */
int xmca_project(xmca_handle* h, int side, const void* V, int64_t N, int64_t m, int is_complex, void* U_out,
                 int* out_is_complex);

/* MCA.predict on new data (xmca/array.py:1299-1428, ABI 11): out (T_new x q) = (((X[:, keep] - mean) / std) V[:, :m]) W.
 *   X         T_new x N_full row-major new data, host memory, element type `dtype` (the model's real field dtype)
 *   keep_idx  N_keep increasing column indices (int64) of the grid points kept by the model; NULL: all N_full = N_keep columns
 *   mean, std N_keep values of `dtype`; std == NULL: no division.  Subtraction and division run in `dtype`, the host's
 *             `x -= mean; x /= std` bit for bit
 *   V         N_keep x m host float64 / interleaved complex128 (v_is_complex), or NULL: the first m resident vectors of the last
 *             solve of `side` (the product then runs in their precision: float32 vectors of a real float32 field stay float32)
 *   W         m x q float64 / interleaved complex128 (w_is_complex) mixing matrix, host memory (the caller's 1/sqrt(sigma), inverse
 *             rotation, mode order and selection)
 *   out       T_new x q float64, interleaved complex128 when *out_is_complex = 1 (V or W complex)
 * Rows are processed in blocks of bounded size.  The resident fields and vectors are not changed. */
int xmca_predict(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int dtype, const int64_t* keep_idx,
                 int64_t N_keep, const void* mean, const void* std, const void* V, int v_is_complex, const double* W, int64_t m,
                 int64_t q, int w_is_complex, double* out, int* out_is_complex);

/* MCA.reconstructed_fields / _reconstructed_X (xmca/array.py:1263-1292, ABI 11): out (T x N_full, float64, row-major).  Kept
 * column keep_idx[c] = Re(B V[:, :m]^H)[:, c], times std[c] when std != NULL, plus mean[c] when mean != NULL; every other column
 * NaN.  keep_idx == NULL with N_full == N_keep: the compact T x N_keep result.
 *   B         T x m float64 / interleaved complex128 (b_is_complex) coefficients, host memory; m == 0: a zero product
 *   V         N_keep x m host float64 / interleaved complex128 (v_is_complex), or NULL: the first m resident vectors of `side`
 *   mean, std N_keep float64 values or NULL
 * Rows are processed in blocks of bounded size.  The resident fields and vectors are not changed. */
int xmca_reconstruct(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V, int v_is_complex,
                     const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean, const double* std, double* out);

/* xmca_predict with per-grid-point weights - the `data *= coslat weights` of xMCA._scale_X (xmca/xarray.py:97-108; an entry point
 * added to ABI 15 - no existing signature changes): out = (((X[:, keep] - mean) / std * weight) V[:, :m]) W.
 *   weight    N_keep float64 values, host memory, applied after `- mean`, `/ std`: the product is formed in double and rounded to
 *             `dtype`, numpy's in-place `x *= w` for a float64 w bit for bit (a plain multiply for XMCA_F64).  NULL: xmca_predict,
 *             to the bit
 * Every other argument as in xmca_predict. */
int xmca_predict_weighted(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int dtype, const int64_t* keep_idx,
                          int64_t N_keep, const void* mean, const void* std, const void* V, int v_is_complex, const double* W, int64_t m,
                          int64_t q, int w_is_complex, double* out, int* out_is_complex, const double* weight);

/* xmca_reconstruct with the weights taken out again - the `field /= coslat weights` of xMCA._scale_X_inverse (xmca/xarray.py:110-126;
 * an entry point added to ABI 15 - no existing signature changes): kept column keep_idx[c] = Re(B V[:, :m]^H)[:, c] / inv_weight[c],
 * then `* std[c]` and `+ mean[c]` as in xmca_reconstruct.
 *   inv_weight  N_keep float64 values, host memory.  The division is IEEE, never a multiplication by a reciprocal: a weight of 0
 *               gives inf / NaN as numpy does.  NULL: xmca_reconstruct, to the bit
 * Every other argument as in xmca_reconstruct. */
int xmca_reconstruct_weighted(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V,
                              int v_is_complex, const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean,
                              const double* std, double* out, const double* inv_weight);

/* xmca_predict_weighted for new data in either memory space (an entry point added to ABI 15 - no existing signature changes).
 *   x_location  XMCA_HOST: X is contiguous host memory (stride_t = N_full, stride_n = 1): xmca_predict_weighted, to the bit.
 *               XMCA_DEVICE: X is memory of the handle's GPU, element (t, n) at X[t * stride_t + n * stride_n] (strides in
 *               elements, not negative).  It is not staged: with stride_n == 1 the ingest reads the rows in place with their
 *               pitch, any other view is made contiguous block by block with the kernels of xmca_set_field_strided.  X is
 *               never written.
 * `out` stays host memory (T_new x q).  Every other argument as in xmca_predict_weighted. */
int xmca_predict_strided(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int64_t stride_t, int64_t stride_n,
                         int x_location, int dtype, const int64_t* keep_idx, int64_t N_keep, const void* mean, const void* std,
                         const void* V, int v_is_complex, const double* W, int64_t m, int64_t q, int w_is_complex, double* out,
                         int* out_is_complex, const double* weight);

/* xmca_reconstruct_weighted with the memory space of `out` as an argument (an entry point added to ABI 15 - no existing signature
 * changes).  out_location XMCA_HOST: xmca_reconstruct_weighted, to the bit.  XMCA_DEVICE: `out` is memory of the handle's GPU
 * (T x N_full float64); the epilogue of every row block writes its rows of `out` directly.  The handle's stream is synchronised
 * before the call returns. */
int xmca_reconstruct_to(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V,
                        int v_is_complex, const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean,
                        const double* std, double* out, const double* inv_weight, int out_location);

/* Correlation maps of MCA.homogeneous_patterns / heterogeneous_patterns (xmca/array.py:1188-1261, the Pearson
 * correlation of tools/array.py:76-88): r[n][j] = corr(real part of field column n of `side`, Y[:, j]) on the resident
 * field - one tall GEMM X^T Y plus column moments instead of the reference's (N + m)^2 corrcoef matrix.
 *   Y      T x m row-major float64 (the real parts of the PCs), host memory
 *   r_out  N x m row-major float64, clamped to [-1, 1] as np.corrcoef clips; NaN (a constant column) stays NaN
 * The field is expected centered, as every caller has it: the one-pass variance loses about (mean / std)^2 eps otherwise.
 * p-values (scipy.stats.beta) stay with the caller. */
int xmca_correlate(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, double* r_out);

/* Two-sided p-values of Pearson correlations of n_obs samples under the exact null distribution (ABI 13): the
 * `2 * scipy.stats.beta(n/2 - 1, n/2 - 1, loc=-1, scale=2).cdf(-abs(r))` of tools/array.py:86-88,
 * p = 2 I_x(a, a) with a = n_obs / 2 - 1 and x = (1 - |r|) / 2, the regularised incomplete beta function by its continued fraction,
 * one value per lane in float64 (csrc/kernels.h pearson_two_sided_p; accuracy: DESIGN.md 2).
 *   r      `count` float64 correlations, host memory;  p_out  `count` float64, host memory
 *   n_obs  3 <= n_obs <= 1 000 000: XMCA_ERR_INVALID below (the distribution does not exist), XMCA_ERR_UNSUPPORTED above
 * NaN stays NaN; |r| >= 1, an ulp beyond included, is exactly 0; p <= 1; values below the normal range go quietly to a denormal or 0.
 * The resident fields and vectors are not changed. */
int xmca_pearson_pvalues(xmca_handle* h, const double* r, int64_t count, int64_t n_obs, double* p_out);
/* The constant of a call of the kernel above, -ln a - ln B(a, a) for a = n_obs / 2 - 1, computed once on the host and passed to
 * every lane (no handle, no device: exported for the host tests).  XMCA_ERR_INVALID outside 3 <= n_obs <= 1 000 000. */
int xmca_pvalue_log_norm(int64_t n_obs, double* out);

/* MCA.homogeneous_patterns / heterogeneous_patterns of one field in their final layout (xmca/array.py:1188-1261, ABI 13): the
 * correlations of xmca_correlate (the same launches), rounded to `r_dtype`, their p-values as xmca_pearson_pvalues with n_obs = T
 * computed from the ROUNDED r - the reference's p belongs to the r it returns - and both maps scattered to N_full x m row-major
 * with NaN at the masked grid points.
 *   Y         T x m row-major float64 (the real parts of the PCs), host memory; 3 <= T <= 1 000 000 (errors as above)
 *   keep_idx  N increasing row indices (int64) below N_full, N the columns of the resident field: the grid points the model kept;
 *             NULL: N_full = N, no masked points
 *   r_out     N_full x m of `r_dtype` (XMCA_F32 / XMCA_F64);  p_out  N_full x m float64;  host memory
 * A constant column gives NaN in both maps.  The resident fields and vectors are not changed. */
int xmca_correlation_maps(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, const int64_t* keep_idx, int64_t N_full,
                          int r_dtype, void* r_out, double* p_out);

/* xmca_correlation_maps with the memory space of both outputs as an argument (an entry point added to ABI 15 - no existing
 * signature changes).  out_location XMCA_HOST: xmca_correlation_maps, to the bit.  XMCA_DEVICE: r_out and p_out are memory of the
 * handle's GPU, written directly by the final kernel.  Y stays host memory.  The handle's stream is synchronised before the call
 * returns. */
int xmca_correlation_maps_to(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, const int64_t* keep_idx, int64_t N_full,
                             int r_dtype, void* r_out, double* p_out, int out_location);

/* Constructor preprocessing on the device (xmca/array.py:199-215 `_set_field_means` / `_set_field_stds` / `_center`;
 * SURVEY 8f row 3): the field of `side` set with xmca_set_field (raw, uncentered) is centered in place, column by
 * column; mean_out / std_out (ddof = 0, float64 accumulation) get N values each and *n_nan_out the number of NaN
 * entries found.  Only the NaN-free columns are centered: a column holding a NaN is left as it is (mean and std NaN), and
 * the caller takes its own NaN-column path when the count is not zero. */
int xmca_center_field(xmca_handle* h, int side, double* mean_out, double* std_out, int64_t* n_nan_out);
/* NaN-column handling of the constructor on the device (xmca/array.py:191-197 `_set_no_nan_idx`, `_remove_nan_cols`,
 * tools/array.py:27-62): keep_out[c] = 1 for every column of the resident raw field of `side` that holds no NaN
 * (N ints), *n_keep_out their number; the resident field is replaced by those columns (T x n_keep, order kept).
 * With n_keep = 0 the field is left as it is (the caller raises the reference's error). */
int xmca_compact_field(xmca_handle* h, int side, int* keep_out, int64_t* n_keep_out);
/* Weights / normalisation of the constructor stage on the device (xmca/array.py:317-349 `apply_weights`, :351-365
 * `normalize`): every column c of the resident real field of `side` is multiplied (divide = 0) or divided (divide = 1)
 * by w[c]; w holds N values of the field's own element type, so the result equals the host operation bit for bit. */
int xmca_scale_field(xmca_handle* h, int side, const void* w, int divide);
/* Real plane of the resident field of `side` (T x N row-major, dtype XMCA_F32 / XMCA_F64 as it was set) -> host. */
int xmca_get_field(xmca_handle* h, int side, void* out);

/* MCA.bootstrapping (xmca/array.py:1813-1952): replicates on the device.
 * xmca_bootstrap_begin copies the real planes of the fields set with xmca_set_field (the caller's X_surr,
 * array.py:1925-1933) into working buffers; they stay as they are until the next xmca_bootstrap_begin. */
int xmca_bootstrap_begin(xmca_handle* h, int n_fields);
/* All replicates of one bootstrap in one call.  idx_left / idx_right: n_runs x T row indices INTO THE FIELDS AS THEY WERE AT
 * xmca_bootstrap_begin - the caller composes the reference's cumulative resampling X <- X[idx_r, :] (its loop overwrites
 * X_surr), c_r = c_{r-1}[idx_r] with idx_r drawn exactly as tools/array.py:91-138 does - or NULL for a side that is not
 * resampled.  The replicates are then independent on the device and several are kept in flight (lanes, as in xmca_rule_n).
 * Replicate r gathers the rows c_r of the working buffers, centers them (the MCA constructor, array.py:117), complexifies when
 * hilbert_col != NULL, solves, rotates (rotated != 0: n_rot = p, power, tol) and contributes the variance spectrum of
 * `_get_variance` (array.py:755-779): n_out = `rank` singular values, or the p sorted norm products of the rotated model.
 * spectra_out: n_runs x n_out; kept_out: n_runs, 0 where Varimax failed. */
int xmca_bootstrap_runs(xmca_handle* h, const double* hilbert_col, const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs,
                        int rotated, int p, int power, double tol, double* spectra_out, int* kept_out, int64_t n_out);
/* xmca_bootstrap_runs of a model solved with extend='exp' (ABI 10): every replicate is complexified with the operator G of
 * xmca_complexify_extended (col3, hbar, U, W, rank for T = the T of xmca_bootstrap_begin) - the reference passes `extend` and
 * `period` into every replicate's solve (xmca/array.py:1935-1947) and resampling rows keeps T, so G is the same for all of them.
 * The fields must be float64 (the reference's replicates are: `_get_X(real=True)` of a complex128 signal); XMCA_ERR_INVALID
 * otherwise. */
int xmca_bootstrap_runs_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W, int rank,
                                 const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p, int power,
                                 double tol, double* spectra_out, int* kept_out, int64_t n_out);
/* Column resampling, `bootstrapping(axis=1)` (ABI 14): the two entries above with column indices in place of row indices.
 * cols_left: n_runs x Nl, cols_right: n_runs x Nr composed indices INTO THE COLUMNS OF [left | right] AS THE FIELDS WERE AT
 * xmca_bootstrap_begin, 0 <= index < Nl + Nr (< Nl with one field; XMCA_ERR_INVALID otherwise, before anything is launched) -
 * the reference resamples the concatenation of both fields with one draw when both sides are resampled and splits it again at
 * Nl (array.py:1921-1928), so a column of either replicate field may come from either working copy; with one side resampled its
 * indices stay inside that side's range (left: c, right: Nl + c).  NULL: the side is copied as it is.  T, Nl and Nr do not
 * change, so the complexification (hilbert_col, or the parts of the extended operator) is the one of the row entries; every
 * replicate is centered again like the MCA constructor does.  Errors and outputs as for the row entries. */
int xmca_bootstrap_runs_columns(xmca_handle* h, const double* hilbert_col, const int64_t* cols_left, const int64_t* cols_right,
                                int64_t n_runs, int rotated, int p, int power, double tol, double* spectra_out, int* kept_out,
                                int64_t n_out);
int xmca_bootstrap_runs_columns_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W,
                                         int rank, const int64_t* cols_left, const int64_t* cols_right, int64_t n_runs, int rotated,
                                         int p, int power, double tol, double* spectra_out, int* kept_out, int64_t n_out);
/* xmca_bootstrap_runs / xmca_bootstrap_runs_columns of a model solved with extend='theta' (entry points added to ABI 15 - no existing
 * signature changes).  col3, hbar, B and period are the arguments of xmca_complexify_theta for T = the T of xmca_bootstrap_begin.
 * The Theta fit is not linear in the column, so nothing of it carries over from the model: every replicate is gathered, centred,
 * FITTED AGAIN by the kernels of csrc/theta.h, and complexified as X_im = G0 X + B C, the arithmetic of xmca_complexify_theta,
 * on its lane's stream.  A lane owns its operator G0, its copy of B and one fit buffer (2 (5 + period) x N float64) per field; the
 * handle keeps none of them after the call.  The stage timers of the call show "resample" and "theta_fit".
 * Refused before anything is launched: the errors of xmca_bootstrap_runs; a missing col3, hbar or B, period < 1 or T < 2 period, and
 * working copies that are not float64 (XMCA_ERR_INVALID: the reference's replicates are float64); no xmca_bootstrap_begin
 * (XMCA_ERR_STATE); T above the bound of the T x T assembly (XMCA_ERR_UNSUPPORTED).  Outputs as for the entries above. */
int xmca_bootstrap_runs_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period,
                              const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p, int power,
                              double tol, double* spectra_out, int* kept_out, int64_t n_out);
int xmca_bootstrap_runs_columns_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period,
                                      const int64_t* cols_left, const int64_t* cols_right, int64_t n_runs, int rotated, int p,
                                      int power, double tol, double* spectra_out, int* kept_out, int64_t n_out);
/* Bootstrap mean and standard error of the k leading singular vectors (an extension), after xmca_bootstrap_begin.
 * Replicate r gathers the rows idx[r * T .. (r + 1) * T) of EVERY working copy (a pairs bootstrap; independent draws, not
 * composed), is centred, complexified with the Hilbert transform (hilbert_col; NULL: real) and solved for its k leading vectors
 * v_r.  With the model's unit vectors v0 (host float64 planes of k x N[side], mode-major; the im planes NULL for a real model, the
 * right ones NULL for one field):  c_rj = sum over sides and columns of conj(v0[j, n]) v_r[j, n];  u_rj = conj(c_rj) / |c_rj|
 * (1 where c_rj = 0);  d = u_rj v_r - v0;  S = sum_r d and Q = sum_r |d|^2 in float64.
 *   mean_*        k x N[side] float64, interleaved (re, im) when complex:  v0 + S / n_runs
 *   std_*         k x N[side] float64:  sqrt(max(0, Q - |S|^2 / n_runs) / (n_runs - 1))
 *   congruence_out  n_runs x k:  |c_rj| / n_fields, in [0, 1]
 *   sigma_out     n_runs x k: the replicates' leading singular values;  kept_out  n_runs flags (always 1: nothing is rotated)
 * No sum uses an atomic: a call repeats its bits.  The association of S and Q follows the lanes the runs fall on
 * (XMCA_RULE_N_LANES), so two lane counts agree to rounding; congruence_out and sigma_out do not depend on the lanes.
 * Refused before anything is launched (XMCA_ERR_INVALID): n_runs < 2, k < 1 or above min(T, N), an index outside [0, T), missing
 * vectors or outputs; no xmca_bootstrap_begin: XMCA_ERR_STATE. */
int xmca_bootstrap_patterns(xmca_handle* h, const double* hilbert_col, const int64_t* idx, int64_t n_runs, int k,
                            const double* v0_left_re, const double* v0_left_im, const double* v0_right_re, const double* v0_right_im,
                            double* mean_left, double* std_left, double* mean_right, double* std_right, double* congruence_out,
                            double* sigma_out, int* kept_out);
/* (tests) The statistics of xmca_bootstrap_patterns from replicate vectors given by the host: v_* are n_runs x k x N[side] float64
 * planes, narrowed to float32 on the device when plane_dtype is XMCA_F32; N_right = 0: one side.  Run r is accumulated in the
 * accumulators r % n_lanes (1 <= n_lanes <= 8), which are then merged as the lanes of a bootstrap are.  Outputs as above. */
int xmca_pattern_stats(xmca_handle* h, const double* v0_left_re, const double* v0_left_im, const double* v0_right_re,
                       const double* v0_right_im, const double* v_left_re, const double* v_left_im, const double* v_right_re,
                       const double* v_right_im, int64_t n_runs, int k, int64_t N_left, int64_t N_right, int is_complex, int plane_dtype,
                       int n_lanes, double* mean_left, double* std_left, double* mean_right, double* std_right,
                       double* congruence_out);
/* (no device) Columns per partial sum of the alignment c_rj: a compile-time constant, so the association of that sum is a
 * function of N alone. */
int xmca_pattern_tile(void);

/* Extended EOF analysis (lag-embedded EOFs; an extension; entry points added to ABI 15 - no existing signature
 * changes).  With X the resident real T x N field of side 0 as solve() sees it, M = embedding, T' = T - (M - 1) tau and
 * X_j = X[j tau : j tau + T', :], the analysis is the SVD of Y = [X_0 | ... | X_{M-1}] with every column centred over its T' rows.
 * Y is never formed: its Gram matrix is K[t][s] = sum_{j < M} G[t + j tau][s + j tau] of G = X X^T, the centring is the double
 * centring K_c = H K H (H = I - 1 1^T / T'), the patterns of lag j are X_j^T u_c / sigma_c.
 *   xmca_extended_eofs  Gram product, lag sum and centring (csrc/lag_gram.h), the n_modes leading eigenvectors of K_c (the partial
 *                       eigensolver of solve(n_modes=k), with its guard at the cut), one back-projection per lag on a row-offset view
 *                       of the field with 1 / sigma_c in the product's epilogue, sign, final layout.
 *     keep_idx, N_full  as in xmca_get_maps: N increasing row indices below N_full, every other row of a pattern NaN; NULL: N_full = N
 *     lam_out           T' float64: all eigenvalues of K_c (sigma^2), descending
 *     pcs_out           T' x n_modes float64, row-major: u_c sqrt(T' - 1)
 *     eofs_out          embedding x N_full x n_modes float64: slice j the patterns at lag j tau; unit norm over lags x points
 *                       Sign of mode c: the entry of largest magnitude of its lag-0 pattern is positive (the first one on a tie).
 *                       XMCA_ERR_INVALID: embedding or tau < 1, T' < 2, n_modes outside [1, min(T' - 1, M N)], a complex resident field;
 *                       XMCA_ERR_STATE: no field.  The call works in buffers of its own: the result of a solve, its rotation, a
 *                       back-projection tail and the field planes are left as they are.  Stage timers: "gram", "lag_gram",
 *                       "eeof_eigh", "eeof_project", "eeof_assemble".  No sum uses an atomic: a call repeats its bits.
 *   xmca_lag_gram       (tests) the lag-sum and centring kernels alone on a host n x n float64 matrix G (symmetric): K_out,
 *                       T' x T' with T' = n - (embedding - 1) tau >= 1, is the lag sum (terms added in the order j = 0 .. M-1) and,
 *                       with center != 0, its double centring K - (r_t + r_s) + g from the means r of its columns and their mean g.
 *   xmca_lag_gram_tile  (no device) the output tile edge of the lag-sum kernel.  A tile's M shifted windows are staged through LDS as
 *                       one diagonal band when tau is below the tile edge and tile + (M - 1) tau <= 96 rows; plain row reads otherwise. */
int xmca_extended_eofs(xmca_handle* h, int embedding, int tau, int n_modes, const int64_t* keep_idx, int64_t N_full, double* lam_out,
                       double* pcs_out, double* eofs_out);
int xmca_lag_gram(xmca_handle* h, const double* G, int64_t n, int embedding, int tau, int center, double* K_out);
int xmca_lag_gram_tile(void);

/* Reconstructed components of extended EOFs (an extension; entry points added to ABI 15 - no existing signature
 * changes).  Notation as above; mu the row of column means of Y, Y^ = sum over the selected modes of s_k u_k v_k^T.  With
 * J(t) = { j : 0 <= j < M, 0 <= t - j tau < T' } and c_t = |J(t)|, the reconstructed component on the T time steps of the field is
 * R[t][n] = (1 / c_t) sum_{j in J(t)} Y^[t - j tau][j N + n], the diagonal averaging of Y^, and m[t][n] the same average of mu.
 *   xmca_extended_reconstruct  the front of xmca_extended_eofs (the leading modes[n_sel - 1] + 1 eigenvectors), then
 *                       R = diag(1 / c) A~ P with A~ from lag_expand_kernel and P the back-projections Z_sel X_j of the uncentred
 *                       windows (no division by sigma, no sign), as one product per block of rows into the finish of
 *                       xmca_reconstruct_to:  out (T x N_full, float64) = ((R + m) / inv_weight) * std + mean, NaN at the columns
 *                       not in keep_idx.  add_means == 0 leaves m out; mean, std, inv_weight (N_keep values each) may be NULL.
 *     modes             n_sel 0-based, strictly increasing mode indices below min(T' - 1, M N)
 *     keep_idx, N_keep, N_full, out, out_location   as in xmca_reconstruct_to; N_keep is the number of columns of the field
 *                       XMCA_ERR_INVALID: embedding or tau < 1, T' < 2, tau > T' with embedding > 1 (time steps in no window),
 *                       n_sel < 1, modes unsorted or out of range, a complex resident field;  XMCA_ERR_STATE: no field.  The call
 *                       works in buffers of its own: the result of a solve, its rotation, a back-projection tail and the field
 *                       planes are left as they are.  Stage timers: those of xmca_extended_eofs up to "eeof_project", then
 *                       "eeof_expand", "eeof_window_means", "eeof_reconstruct".  No sum uses an atomic: a call repeats its bits.
 *   xmca_lag_expand     (tests) lag_expand_kernel alone: from the host q x Tp float64 matrix Z (row c one vector), A_out is
 *                       T x embedding (q + 1) (with_indicators != 0) or T x embedding q, T = Tp + (embedding - 1) tau, row-major:
 *                       A[t][j q + c] = Z[c][t - j tau] inside window j, else 0; A[t][embedding q + j] = 1 inside window j, else 0;
 *                       inv_count_out[t] = 1 / c_t.  XMCA_ERR_INVALID: tau > Tp with embedding > 1.
 *   xmca_lag_window_means  (tests) the means of the embedding windows of every column of the resident field of side 0,
 *                       embedding x N float64: one pass over the field, rows cut at the window boundaries and summed in increasing
 *                       order in float64 (a float32 field too). */
int xmca_extended_reconstruct(xmca_handle* h, int embedding, int tau, const int* modes, int n_sel, int add_means,
                              const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean, const double* std,
                              const double* inv_weight, double* out, int out_location);
int xmca_lag_expand(xmca_handle* h, const double* Z, int q, int Tp, int embedding, int tau, int with_indicators, double* A_out,
                    double* inv_count_out);
int xmca_lag_window_means(xmca_handle* h, int embedding, int tau, double* means_out);

/* Monte-Carlo SSA test of extended EOFs (Allen & Smith 1996; an extension; entry points added to ABI 15 - no existing
 * signature changes).  Notation as above; H Y = U S V^T, lambda_k = s_k^2, v_k = Y^T u_k / s_k the unit-norm patterns of
 * xmca_extended_eofs.  For a surrogate field R (T x N) with the embedded matrix Y_R, the statistic of mode k is
 * Lambda_k(R) = || H Y_R v_k ||^2: with V_j (N x n_modes) the lag-j patterns and W = R [V_0 | ... | V_{M-1}] (T x M n_modes, one
 * thin product over the whole surrogate), Q[t][c] = sum_{j < M} W[t + j tau][j n_modes + c] and Lambda_c = sum_t (Q[t][c] -
 * mean_t Q[.][c])^2 (csrc/lag_project.h).  Neither Y_R nor a T x T matrix is formed, and no surrogate is decomposed.
 * Lambda_k(X) = lambda_k.  The null is one AR(1) series per column: column c of R is the unit-variance series of
 * xmca_surrogate_ar1 - the same generator, segments and key (seed, run, side = 0) - times d_c, the sample standard deviation
 * (ddof = 1) of column c of the resident field; d is folded into the patterns once (W = R (diag(d) V)), the surrogate is never
 * rescaled.  No bias correction of phi or d is applied.
 *   xmca_extended_rule_n   the front of xmca_extended_eofs and its patterns once, then for every run of [run_begin, run_end): the
 *                       surrogate in a buffer of the call's own, the product, the projection; the values stay on the device until
 *                       the one download at the end.
 *     phi               N host float64, every one finite with |phi| < 1 (checked before anything is launched)
 *     lam_out           T' float64: all eigenvalues of K_c, descending (those of xmca_extended_eofs)
 *     scale_out         N float64: d_c
 *     surrogates_out    (run_end - run_begin) x n_modes float64, row-major: Lambda_c of every run
 *                       Errors as xmca_extended_eofs, and XMCA_ERR_INVALID for a bad run range or phi.  The call works in buffers
 *                       of its own: a resident field, the result of a solve, its rotation and a back-projection tail are left as
 *                       they are.  Stage timers: those of xmca_extended_eofs up to "eeof_project", then "mcssa_scale",
 *                       "mcssa_surrogate", "mcssa_gemm", "mcssa_project".  No sum uses an atomic: a call repeats its bits, and a
 *                       run's values do not depend on the range it is part of.
 *   xmca_extended_project  (tests) the same front and the same scale, product and projection kernels applied to the host T x N
 *                       float64 field R, narrowed to the resident field's dtype: out (n_modes) = Lambda_c(R), with d folded in
 *                       when apply_scale != 0.  R = the field and apply_scale == 0 give lambda_c.
 *   xmca_lag_project    (tests) the projection kernels alone on a host T x embedding k float64 matrix W: out (k) = Lambda_c.
 *   xmca_lag_project_tile  (no device) rows and columns of Q one workgroup of the projection kernels handles. */
int xmca_extended_rule_n(xmca_handle* h, int embedding, int tau, int n_modes, const double* phi, int64_t run_begin, int64_t run_end,
                         uint64_t seed, double* lam_out, double* scale_out, double* surrogates_out);
int xmca_extended_project(xmca_handle* h, int embedding, int tau, int n_modes, const double* R, int apply_scale, double* out);
int xmca_lag_project(xmca_handle* h, const double* W, int64_t T, int embedding, int tau, int k, double* out);
int xmca_lag_project_tile(int* rows_out, int* cols_out);

/* DINEOF gap filling of one real field (an extension; entry points added to ABI 15 - no existing signature changes).
 * X is T x N in `dtype`, NaN marks a missing value.  Every column is centred over its present values (float64 sums in a fixed
 * order), missing entries start at 0 and are replaced, iteration after iteration, by the truncated reconstruction of the plane A:
 * G = A A^T, Z its n_modes leading eigenvectors (the partial eigensolver of solve(n_modes=k)), P = Z A, A[t][n] = sum_c Z[c][t]
 * P[c][n] at the masked entries only.  d_i = sqrt(sum of the squared changes / masked entries) / scale, scale the RMS of the present
 * anomalies; the loop ends with d_i < tol or after max_iter iterations (tol = 0: exactly max_iter).
 *   xmca_fill_gaps      cv_idx, n_cv   flat indices into X of present entries that are withheld (treated as missing) during the
 *                                      iteration and restored afterwards; NULL, 0: none
 *                       out            T x N in `dtype`: X with its missing entries filled (reconstruction + column mean); present
 *                                      and withheld entries keep the bits of X
 *                       history_out    max_iter float64: d_1 .. d_iters (the rest is not written);  iters_out: iterations run
 *                       cv_rms_out     RMS over the withheld entries of (filled - true) in the units of X; NaN without any
 *                       lam_out        the n_modes leading eigenvalues of G of the last iteration
 *                       XMCA_ERR_INVALID, before anything is launched: n_modes outside [1, min(T, N) - 1], max_iter < 1, tol
 *                       negative or not finite, a column without a finite value, an Inf in X, a cv_idx entry out of range,
 *                       repeated or pointing at a NaN.  XMCA_ERR_NUMERIC: the present anomalies have no variance.  The call works
 *                       in buffers of its own: a resident field, the result of a solve, its rotation and a back-projection tail
 *                       are left as they are.  Stage timers: "gap_center", "gram", "gap_eigh", "gap_project", "gap_fill",
 *                       "gap_finish".  No sum uses an atomic: a call repeats its bits.
 *   xmca_gap_center     (tests) the centring and mask kernels alone on a host field: the N column means, the T x N mask bytes
 *                       (0 present, 1 missing), the centred plane widened to float64 (0 at the missing entries) and scale.
 *   xmca_gap_fill_step  (tests) the fill kernel alone on host inputs: A (T x N in `dtype`), mask bytes (non-zero: fill), Z
 *                       (n_modes x T) and P (n_modes x N) in float64; A_out is the updated plane, sum_out the sum of the squared
 *                       changes.  Entries with a zero mask byte come back with their bits.
 *   xmca_gap_fill_tile  (no device) rows and columns of a tile of the fill kernel: one workgroup per tile, one lane per column,
 *                       P in registers in chunks of 16 modes, the Z values of 16 rows at a time through LDS. */
int xmca_fill_gaps(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, const int64_t* cv_idx, int64_t n_cv, int n_modes,
                   int max_iter, double tol, void* out, double* history_out, int* iters_out, double* cv_rms_out, double* lam_out);
int xmca_gap_center(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, double* mean_out, unsigned char* mask_out,
                    double* A_out, double* scale_out);
int xmca_gap_fill_step(xmca_handle* h, const void* A, const unsigned char* mask, const double* Z, const double* P, int64_t T, int64_t N,
                       int n_modes, int dtype, void* A_out, double* sum_out);
int xmca_gap_fill_tile(int* rows_out, int* cols_out);

/* M-SSA gap filling (Kondrashov & Ghil 2006; an extension; entry points added to ABI 15 - no existing signature
 * changes): the iteration of xmca_fill_gaps on the lag-embedded plane [A_0 | ... | A_{M-1}], A_j = A[j tau : j tau + T', :],
 * T' = T - (embedding - 1) tau, so that a value is rebuilt from its neighbours in time as well as in space and a time step without
 * any present value is bridged.  Plane, mask, column means and scale are those of xmca_fill_gaps, formed once; nothing is centred
 * again.  Iteration: G = A A^T, K = sum_j G[j tau : j tau + T', j tau : j tau + T'] (the lag sum of xmca_lag_gram, not centred),
 * Z the n_modes leading eigenvectors of K (n_modes x T'), P_j = Z A_j, and at the masked entries only
 * A[t][n] = (1 / c_t) sum_{j in J(t)} sum_c Z[c][t - j tau] P_j[c][n], J(t) = { j : 0 <= t - j tau < T' }, c_t = |J(t)|: the
 * diagonally averaged rank-n_modes truncation of the embedded plane, which is never formed.
 *   xmca_fill_gaps_lagged   the arguments of xmca_fill_gaps and embedding, tau; lam_out: the n_modes leading eigenvalues of K of the
 *                       last iteration.  embedding == 1 is xmca_fill_gaps to the bit (tau is not looked at).  XMCA_ERR_INVALID,
 *                       before anything is launched: what xmca_fill_gaps refuses, embedding or tau below 1, and with embedding > 1:
 *                       T' < 2, tau > T' (time steps in no window), n_modes outside [1, min(T', embedding N) - 1].  Stage timers:
 *                       those of xmca_fill_gaps and "gap_lag_gram".
 *   xmca_gap_lag_fill_step  (tests) the lagged fill kernel alone on host inputs: A (T x N in `dtype`), mask bytes (non-zero: fill),
 *                       Z (n_modes x T') and P (embedding n_modes x N, row j n_modes + c the lag-j pattern of mode c) in float64;
 *                       A_out is the updated plane, sum_out the sum of the squared changes.  Entries with a zero mask byte come
 *                       back with their bits.  XMCA_ERR_INVALID: T' < 1, or tau > T' with embedding > 1. */
int xmca_fill_gaps_lagged(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, const int64_t* cv_idx, int64_t n_cv, int n_modes,
                          int embedding, int tau, int max_iter, double tol, void* out, double* history_out, int* iters_out,
                          double* cv_rms_out, double* lam_out);
int xmca_gap_lag_fill_step(xmca_handle* h, const void* A, const unsigned char* mask, const double* Z, const double* P, int64_t T, int64_t N,
                           int n_modes, int embedding, int tau, int dtype, void* A_out, double* sum_out);

/* Column regression: seasonal cycle and trend removed on the device (an extension; entry points added to ABI 15 -
 * no existing signature changes).  Every column of the T x N field X (NaN = missing) is fitted by least squares on the k columns
 * of `basis` (T x k float64, row-major, host memory) over its present entries, in float64 whatever `dtype`:
 * (sum_present b_t b_t^T) c = sum_present b_t x_t, by Cholesky in the order of the basis columns.  A column is FITTED when it has at
 * least k present entries and every pivot d_j = A[j][j] - sum_{i<j} L[j][i]^2 exceeds 1e-8 A[j][j]; the residual x - B c, one
 * float64 fma chain c = 0 .. k-1 from x rounded once to `dtype`, replaces its present entries.  Missing entries and the columns
 * that are not fitted come back NaN.
 *   X, in_location      XMCA_HOST: contiguous host memory (the strides are not looked at);  XMCA_DEVICE: memory of the handle's GPU,
 *                       element (t, n) at X[t * stride_t + n * stride_n] (strides in elements, >= 0), copied by the kernels of
 *                       xmca_set_field_strided into a buffer of this call - the caller's memory is only read
 *   xmca_column_regress field_out, out_location  T x N in `dtype`, contiguous: host memory, or (XMCA_DEVICE, as xmca_correlation_maps_to)
 *                       memory of the handle's GPU that the residual kernel writes directly
 *                       coef_out       k x N float64 (host): the coefficients, NaN where the column is not fitted
 *                       fitted_out     N bytes (host): 1 fitted, 0 not
 *                       XMCA_ERR_INVALID, before anything is launched: k outside [1, 16], T < 1, N < 1, a bad dtype or location, a
 *                       negative stride, a device pointer that is none of the handle's GPU.  Not checked: an Inf in X (the caller's).
 *                       The call works in buffers of its own: a resident field, the result of a solve, its rotation and a
 *                       back-projection tail are left as they are.  Stage timers: "reg_mask", "reg_moments", "reg_solve",
 *                       "reg_residual" (and "ingest_strided" for a device field).  No sum uses a floating-point atomic: a call
 *                       repeats its bits.
 *   xmca_column_residual  the residual step alone with given coefficients `coef` (k x N float64, host; a column with a NaN among
 *                       its k values counts as not fitted): with the basis and coefficients of xmca_column_regress, the bits of
 *                       its field_out.
 *   xmca_reg_mask       (tests) the mask / widen pass alone on a host field: the T x N mask bytes (0 present, 1 missing), the plane
 *                       widened to float64 (0 at the missing entries) and the number of missing entries.
 *   xmca_reg_solve      (tests) the solve kernel alone on host moments: `normal` holds k (k + 1) / 2 + 1 rows - the packed lower
 *                       triangle, entry (i, j <= i) at row i (i + 1) / 2 + j, then the number of present entries - of N float64
 *                       values each, or of one value each when shared_normal != 0 (one matrix for every column); rhs k x N.
 *   xmca_reg_residual_tile  (no device) rows and columns of a tile of the residual kernel: one workgroup per tile, one lane per
 *                       column with its k coefficients in registers, the basis rows of the tile through LDS. */
int xmca_column_regress(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                        const double* basis, int k, void* field_out, int out_location, double* coef_out, unsigned char* fitted_out);
int xmca_column_residual(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                         const double* basis, int k, const double* coef, void* field_out, int out_location);
int xmca_reg_mask(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, unsigned char* mask_out, double* wide_out,
                  int64_t* missing_out);
int xmca_reg_solve(xmca_handle* h, const double* normal, int shared_normal, const double* rhs, int64_t N, int k, double* coef_out,
                   unsigned char* fitted_out);
int xmca_reg_residual_tile(int* rows_out, int* cols_out);

/* Time filter: a gap-aware FIR filter along time on the device (an extension; entry points added to ABI 16 - no
 * existing signature changes).  With L = n_weights = 2 h + 1 weights w (float64, host memory; any finite values, symmetric or not)
 * the smoother of the T x N field X (NaN = missing) is the correlation S[t][n] = sum_{k < L} w[k] X[t + k - h][n] - w[0] meets the
 * earliest step - accumulated in float64 whatever `dtype` as one fma chain in ascending k that starts from +0.0.  The output is S,
 * or X - S with complement != 0, rounded once to `dtype`.
 *   renormalise == 0    strict: an output entry is NaN exactly when one of the L entries of its window is missing or lies outside
 *                       the record (so the first and last h rows are NaN).  trim != 0 returns only the T - 2 h rows h .. T - h - 1,
 *                       with the bits they have without trim; it needs T >= L.  den_min is not looked at.
 *   renormalise != 0    S = num / den, the same ascending chains of w[k] x and of w[k] over the PRESENT entries of the window, steps
 *                       outside the record counting as missing.  An output entry is NaN exactly when X[t][n] itself is missing or
 *                       den < den_min.  The caller forms den_min = min_weight * sum(w) once in float64; it needs sum(w) > 0 (summed
 *                       in ascending k), 0 < den_min <= sum(w) and trim == 0.
 *   X, in_location      XMCA_HOST: contiguous host memory (the strides are not looked at);  XMCA_DEVICE: memory of the handle's GPU,
 *                       element (t, n) at X[t * stride_t + n * stride_n] (strides in elements, >= 0), copied by the kernels of
 *                       xmca_set_field_strided into a buffer of this call - the caller's memory is only read
 *   field_out, out_location  (trim ? T - 2 h : T) x N in `dtype`, contiguous: host memory, or (XMCA_DEVICE, as xmca_column_regress)
 *                       memory of the handle's GPU that the filter kernel writes directly
 *   XMCA_ERR_INVALID, before anything is launched: n_weights even or outside [1, 1025], a weight that is not finite, T < 1, N < 1,
 *                       a bad dtype or location, a negative stride, trim with T < L or with renormalise, renormalise with
 *                       sum(w) <= 0 or den_min outside (0, sum(w)], a device pointer that is none of the handle's GPU.  Not
 *                       checked: an Inf in X (the caller's).  XMCA_ERR_UNSUPPORTED: the size limits of xmca_column_regress.
 *                       The call works in buffers of its own: a resident field, the result of a solve, its rotation and a
 *                       back-projection tail are left as they are.  Stage timers: "time_filter" (and "ingest_strided" for a device
 *                       field).  One kernel reads X in its own type and writes the result - no mask plane, no widened plane, no
 *                       floating-point atomic, no scratch memory: a call repeats its bits.
 *   xmca_time_filter_tile  (no device) output rows and columns of a workgroup's tile of the filter kernel - one lane per column with
 *                       the accumulators of its rows in registers, the weights in LDS, the rows of the tile and its 2 h halo rows
 *                       streamed once - and the most weights a call takes. */
int xmca_time_filter(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                     const double* weights, int n_weights, int complement, int renormalise, double den_min, int trim, void* field_out,
                     int out_location);
int xmca_time_filter_tile(int* rows_out, int* cols_out, int* max_weights_out);

/* Lead-lag maps: regression and correlation of every column of a field with gaps on index series at a list of lags, on the device
 * (an extension; entry points added to ABI 16 - no existing signature changes).  X is the T x N field (NaN =
 * missing), Y the T x q plane of the CENTRED index series (float64, host memory, row-major, finite; 1 <= q <= 8), lags n_lags
 * distinct integers with |lag| <= T - 1 and n_lags * q <= 1024.  For lag l the pairs of column n are (y[s], x[s + l][n]) over the
 * steps s in [max(0, -l), min(T, T - l)) at which x[s + l][n] is present: a positive lag means the index leads the field.  With c_n
 * the mean of the present values of column n (one ascending float64 chain; 0 for an empty column) and x' = x - c_n, the sums
 * n, Sx, Sxx per (lag, column) and Sy, Syy, Sxy per (lag, column, series) are float64 chains in ascending s that start from +0.0,
 * whatever `dtype`; Cxx = Sxx - Sx^2 / n, Cyy = Syy - Sy^2 / n, Cxy = Sxy - Sx Sy / n.  An entry is live exactly when
 * n >= min_pairs, Cxx > 2^-40 Sxx and Cyy > 2^-40 Syy; r = Cxy / sqrt(Cxx Cyy) clamped to [-1, 1] and slope = Cxy / Cyy are rounded
 * once to `dtype`; a dead entry has r, slope and p NaN and dof 0.
 *   dof_mode            XMCA_DOF_N: dof = n;  XMCA_DOF_BRETHERTON: dof = min(n, floor(n f)), f = 1 where rho <= 0 else
 *                       (1 - rho) / (1 + rho), rho = rho_x[n] rho_y[j]; rho_x[n] = [sum_P x'_t x'_{t+1} / |P|] / [sum_present x'^2 /
 *                       n0] over the steps P with x[t] and x[t + 1] present (0 where |P| = 0 or the denominator is not positive;
 *                       clamped to [-1, 1]) is formed on the device, rho_y (q values in [-1, 1], host) is the caller's
 *   p                   pearson_two_sided_p(the rounded r, dof / 2 - 1, log_norm[dof]) with a table of xmca_pvalue_log_norm at
 *                       3 .. T built on the host once per call; NaN where dof < 3
 *   X, in_location, strides   as xmca_time_filter
 *   r_out, slope_out    n_lags x N x q in `dtype`;  p_out n_lags x N x q float64;  dof_out n_lags x N x q int;  pairs_out
 *                       n_lags x N int (every column);  lag1_out N float64, rho_x - required with XMCA_DOF_BRETHERTON, else
 *                       NULL.  All in host memory, or (out_location == XMCA_DEVICE) all in memory of the handle's GPU that the
 *                       kernels write directly.
 *   XMCA_ERR_INVALID, before anything is launched: q outside [1, 8], n_lags < 1, n_lags * q > 1024, a duplicate lag, |lag| >= T,
 *                       min_pairs < 3, a NaN or an Inf in Y, an unknown dof_mode, XMCA_DOF_BRETHERTON without rho_y or lag1_out
 *                       or with a rho_y outside [-1, 1], T < 1, N < 1, a bad dtype or location, a negative stride, a missing
 *                       pointer, a device pointer that is none of the handle's GPU.  Not checked: an Inf in X (the caller's).
 *                       XMCA_ERR_UNSUPPORTED: T above 1 000 000 (the p-value's range), the size limits of xmca_column_regress.
 *                       The call works in buffers of its own: a resident field, the result of a solve, its rotation and a
 *                       back-projection tail are left as they are.  Stage timers: "lead_lag_center", "lead_lag_lag1"
 *                       (XMCA_DOF_BRETHERTON), "lead_lag_moments", "lead_lag_finish" (and "ingest_strided" for a device field).
 *                       No mask plane, no widened plane, no floating-point atomic, no scratch memory: a call repeats its bits,
 *                       and the results of a lag do not depend on the other lags of the call or on their order.
 *   xmca_lead_lag_tile  (no device) the columns of a workgroup of the moment kernel, the rows of a piece a lane loads together, and
 *                       lag_group_out[q - 1], q = 1 .. 8: the lags of a workgroup's group with q index series. */
#define XMCA_DOF_N 0
#define XMCA_DOF_BRETHERTON 1
int xmca_lead_lag_maps(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                       const double* Y, int q, const int* lags, int n_lags, int min_pairs, int dof_mode, const double* rho_y, void* r_out,
                       void* slope_out, double* p_out, int* dof_out, int* pairs_out, double* lag1_out, int out_location);
int xmca_lead_lag_tile(int* cols_out, int* rows_out, int* lag_group_out);

/* Spectral maps: Welch power spectra of every column of a field with gaps, and its cross-spectrum, coherence, phase and gain against
 * index series, on the device (an extension; entry points added to ABI 16 - no existing signature changes).  X is the
 * T x N field (NaN = missing), Y the T x q plane of the CENTRED index series (float64, host memory, row-major, finite; 0 <= q <= 4;
 * NULL with q = 0), L = nperseg in [8, 4096], L <= T, step in [ceil(L / 4), L], weights L finite float64 values with a positive sum of
 * squares, bins n_bins distinct integers in [0, L / 2].  Segment m covers the rows m step .. m step + L - 1, m < K = (T - L) / step + 1;
 * it is present for column n exactly when its L entries are, and K_n counts the present ones.  With c_n the mean of the present
 * values of column n (one ascending float64 chain; 0 for an empty column and with XMCA_DETREND_NONE) and x' = x - c_n, the segment
 * DFT A_k = sum_j (w_j x'_j) (cos t - i sin t), t = 2 pi ((k j) mod L) / L, is one float64 fma chain per part in ascending j from
 * +0.0, whatever `dtype`, with (cos t, -sin t) from a table of L entries built on the host in extended precision and indexed by
 * exact integer arithmetic; Z_k = A_k - mu W_k, mu = (sum_j x'_j) / L and W the DFT of the weights (XMCA_DETREND_MEAN; mu = 0 with
 * XMCA_DETREND_NONE); the energy of the segment e = sum_j (w_j x'_j)^2 - mu (2 sum_j w_j^2 x'_j - mu sum w^2).  The index goes
 * through the same code and gives Y and e_y per segment.  Over the present segments of the column in ascending m:
 * Sxx_k = sum |Z|^2, R = sum e, and per series Syy_k = sum |Y|^2, C_k = sum conj(Y) Z, Ry = sum e_y.  With side_k = 1 at k = 0 and at
 * k = L / 2 of an even L, else 2, and scale_k = side_k / (fs sum w^2 K_n):
 *   power_out           n_bins x N in `dtype`: scale Sxx;  segments_out N int: K_n, every column
 *   index_power_out, cospectrum_out, quadrature_out   n_bins x N x q in `dtype`: scale Syy, scale Re C, scale Im C
 *   coherence_out, phase_out, gain_out                n_bins x N x q in `dtype`: |C|^2 / (Sxx Syy) clamped to [0, 1], atan2(Im C, Re C)
 *                       (the sign of scipy.signal.csd(index, x): negative where the index leads), |C| / Syy
 *   p_out               n_bins x N x q float64: (1 - coherence)^(Ke - 1) = exp((Ke[K_n] - 1) log1p(-coherence)) from the rounded
 *                       coherence, 0 where that is 1; Ke[K] = K / (1 + 2 sum_{j >= 1, j step < L, j < K} (1 - j / K) rho_j^2),
 *                       rho_j = sum_i w_i w_{i + j step} / sum w^2 (Welch 1967), a host table at 0 .. K built once per call; the
 *                       present segments of a gappy column count as contiguous
 *                       A column with K_n < min_segments is NaN in every map.  Coherence, phase, gain and p are NaN as well where
 *                       K_n < 2 or the bin carries no power: unless Sxx > 2^-40 R and Syy > 2^-40 Ry (a definition).
 *                       The q-maps are NULL with q = 0.  All in host memory, or (out_location == XMCA_DEVICE) all in memory of
 *                       the handle's GPU that the kernels write directly.
 *   X, in_location, strides   as xmca_time_filter
 *   XMCA_ERR_INVALID, before anything is launched: q outside [0, 4], nperseg outside [8, 4096] or above T, step outside
 *                       [ceil(L / 4), L], an unknown detrend, n_bins outside [1, L / 2 + 1], a bin outside [0, L / 2], a duplicate
 *                       bin, a NaN or an Inf in the weights or a sum of squares that is not positive, fs not positive and finite,
 *                       min_segments < 1, a NaN or an Inf in Y, T < 1, N < 1, a bad dtype or location, a negative stride, a missing
 *                       pointer, a device pointer that is none of the handle's GPU.  Not checked: an Inf in X (the caller's).
 *                       XMCA_ERR_UNSUPPORTED: the size limits of xmca_column_regress.
 *                       The call works in buffers of its own: a resident field, the result of a solve, its rotation and a
 *                       back-projection tail are left as they are.  Stage timers: "spectral_center" (XMCA_DETREND_MEAN),
 *                       "spectral_index" (q > 0), "spectral_segments", "spectral_finish" (and "ingest_strided" for a device field).
 *                       No mask plane, no widened plane, no atomic, no scratch memory: a call repeats its bits, and the maps of
 *                       a bin do not depend on the other bins of the call or on their order.
 *   xmca_spectral_tile  (no device) the columns of a workgroup of the segment kernel, the rows of a piece a lane loads together, and
 *                       bin_group_out[q], q = 0 .. 4: the bins of a workgroup's group with q index series. */
#define XMCA_DETREND_NONE 0
#define XMCA_DETREND_MEAN 1
int xmca_spectral_maps(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                       const double* Y, int q, int nperseg, int step, const double* weights, int detrend, const int* bins, int n_bins, double fs,
                       int min_segments, void* power_out, void* index_power_out, void* cospectrum_out, void* quadrature_out, void* coherence_out,
                       void* phase_out, void* gain_out, double* p_out, int* segments_out, int out_location);
int xmca_spectral_tile(int* cols_out, int* rows_out, int* bin_group_out);
int xmca_is_complex(xmca_handle* h);
/* 1 when the singular vectors of `side` from the last xmca_solve are resident in float32: a real float32 field decomposed on
 * its dual side (N > T) keeps `_V` in the input's dtype as the reference does (xmca/array.py:584, the dtype of
 * `VLT.conjugate().T`), and xmca_rotate_solved then multiplies float32 vectors by float32 sqrt(singular values) like the
 * reference's host code (array.py:818-822).  Every other result is float64 planes. */
int xmca_vectors_are_f32(xmca_handle* h, int side);
/* Persistent launches of this process (the register-resident tridiagonal reduction, the one-launch Varimax loop) that ran out
 * of their bounded waits because a workgroup never became resident, and were repeated on the launch-per-step path.  All
 * persistent kernels of a device pass one gate (csrc/common.h PersistGate), so this stays 0 unless ANOTHER process holds CUs. */
long long xmca_persistent_giveups(void);
/* Diagnostics of the last solve: for each of the up to three eigen-decompositions (left Gram, right Gram, kernel):
 * info[3*i + 0] = outer sweeps, info[3*i + 1] = tile size, info[3*i + 2] = pair slots (i = 0..2), then
 * info[9 + i]: bit 0 = the eigensolver inserted a Cholesky LR step (graded spectrum), bit 1 = the problem was solved by
 * reduction to tridiagonal form (csrc/tridiag.h: then no sweeps, tile and slots are 0).
 * A caller that passes n > 12 also gets (a caller passing 12 sees no change):
 * info[12 + i] = eigenvectors the eigensolver actually formed for problem i: 0 (values only), the order of the problem, or -
 *   one field solved with 0 < n_vec < order - the k' >= n_vec of the partial eigenvector stage;
 * info[15] = modes whose vectors are resident (the n_vec of the solve, clipped to the rank);
 * info[16 + s] = KiB of the device blocks that hold the vector planes of side s (what is allocated, not a product of shapes).
 * n <= 18.  No signature changes and a library of before fills nothing beyond 12, which reads as "not reported": the ABI number
 * stays as it is. */
int xmca_get_solve_info(xmca_handle* h, int* info, int n);

/* promax / varimax of xmca/tools/rotation.py:84-149, :15-78 on a host loading matrix L (N x p row-major,
 * float64, interleaved complex when is_complex), as built by MCA.rotate (array.py:821-822).
 *   n_left        rows belonging to the left field (array.py:818, :827-828)
 *   varimax_only  1: stop after Varimax (tools.rotation.varimax), 0: full Promax (also for power = 1)
 *   gamma         the `gamma` of tools.rotation.varimax (rotation.py:15, :56-57): 1 = Varimax (what promax / MCA.rotate
 *                 use), 0 = Quartimax; any real value is accepted
 *   B_out         NULL or N x p rotated loadings
 *   R_out/Phi_out p x p (interleaved complex when is_complex); norm_left/right: p column norms of the two
 *                 row blocks of the rotated loadings (array.py:827-828); iters_out: Varimax iterations run.
 * Returns XMCA_ERR_NOT_CONVERGED when max_iter iterations did not satisfy |d - d_old| / d < tol. */
int xmca_rotate_loadings(xmca_handle* h, const double* L, int64_t N, int64_t n_left, int p, int is_complex, int power,
                         double tol, int max_iter, int varimax_only, double gamma, double* B_out, double* R_out,
                         double* Phi_out, double* norm_left, double* norm_right, int* iters_out);

/* MCA.rotate (xmca/array.py:815-833) on the result of the last xmca_solve, without the vectors leaving the device: the
 * loadings V sqrt(sigma) of both fields are stacked (array.py:818-822) from the resident singular vectors, then as
 * xmca_rotate_loadings (full Promax, gamma = 1).  p <= the number of back-projected modes.  Outputs as there
 * (is_complex = xmca_is_complex(h)); XMCA_ERR_NOT_CONVERGED / XMCA_ERR_NUMERIC as there. */
int xmca_rotate_solved(xmca_handle* h, int p, int power, double tol, int max_iter, double* R_out, double* Phi_out,
                       double* norm_left, double* norm_right, int* iters_out);

/* MCA.rule_n surrogate loop (xmca/array.py:1753-1765) for runs [run_begin, run_end): N(0,1) surrogates
 * (Philox4x32-10 keyed by seed, run, side) generated on the device, centered, optionally complexified
 * (hilbert_col != NULL, see xmca_complexify), solved and, when `rotated`, rotated with (p, power, tol); each kept run contributes
 * MCA._get_variance() (array.py:772-779): n_out = rank values (unrotated) or p values (rotated), descending.
 *   spectra_out  (run_end - run_begin) x n_out float64;  kept_out[i] = 0 when run i was dropped because
 *                Varimax did not converge (array.py:1762-1763).
 * The final normalisation svals /= svals.sum(0) / ref.sum() (array.py:1767-1769) is left to the caller
 * because it needs the runs of every rank. */
int xmca_rule_n(xmca_handle* h, int64_t T, int64_t Nx, int64_t Ny, int n_fields, const double* hilbert_col, int rotated,
                int p, int power, double tol, int64_t run_begin, int64_t run_end, uint64_t seed, int dtype,
                double* spectra_out, int* kept_out, int64_t n_out);

/* Run sharding across the GPUs of a node - the only collective of the path (SURVEY 8(b) `mca_comm_*`, 8(e)).  The reference's
 * surrogate loop (xmca/array.py:1753-1765) is serial; its runs are independent, so rank r of `world` takes a contiguous block
 * of run indices on its own GPU and the per-run spectra are combined by ONE ncclAllGather over xGMI (RCCL, bound at run time:
 * XMCA_ERR_UNSUPPORTED when librccl.so.1 cannot be loaded).  One process per GPU, one communicator per handle's device.
 *   xmca_comm_unique_id  rank 0 fills XMCA_COMM_ID_BYTES bytes (an ncclUniqueId); the caller ships them to the other ranks
 *                        (file, MPI, a torch store - the library has no transport of its own besides RCCL).
 *   xmca_comm_create     collective over all `world` ranks (ncclCommInitRank on the device of `h`).
 *   xmca_comm_allgather  recv_host[r * count + i] = send_host[i] of rank r (float64, host buffers; staged through device memory).
 *   xmca_comm_broadcast  `count` float64 of `root` to every rank (used for the seed: every rank must key the generator alike).
 *   xmca_comm_info       rank, world, number of collectives carried out and bytes received in them (bench.py reports these).
 *   xmca_rule_n_sharded  xmca_rule_n for runs [0, n_runs) split over the ranks of `comm` (rank r: runs r*n/world ... as
 *                        xmca_amd/dist.py shard_range), seed taken from rank 0, then the all-gather: every rank receives all
 *                        n_runs x n_out spectra and kept flags - what array.py:1767-1771 normalises.  The generator is keyed by
 *                        (seed, run, side): the result does not depend on `world`. */
#define XMCA_COMM_ID_BYTES 128
typedef struct xmca_comm xmca_comm;
int xmca_comm_unique_id(void* id_out);
int xmca_comm_create(xmca_handle* h, const void* unique_id, int rank, int world, xmca_comm** out);
void xmca_comm_destroy(xmca_comm* c);
const char* xmca_comm_last_error(xmca_comm* c);
int xmca_comm_allgather(xmca_comm* c, const double* send_host, double* recv_host, int64_t count);
int xmca_comm_broadcast(xmca_comm* c, double* buf_host, int64_t count, int root);
int xmca_comm_info(xmca_comm* c, int* rank, int* world, int64_t* collectives, int64_t* bytes);
int xmca_rule_n_sharded(xmca_handle* h, xmca_comm* c, int64_t n_runs, int64_t T, int64_t Nx, int64_t Ny, int n_fields,
                        const double* hilbert_col, int rotated, int p, int power, double tol, uint64_t seed, int dtype,
                        double* spectra_out, int* kept_out, int64_t n_out);

/* Surrogate generator on its own (tests): T*N standard normals of (seed, run, side) as float64 on the host. */
int xmca_surrogate(xmca_handle* h, int64_t n, uint64_t seed, uint32_t run, uint32_t side, double* out);

/* Red-noise (AR(1)) surrogates for the Rule-N test.  Column c of the surrogate of (run, side) is
 *   x[0] = e[0],  x[t] = phi_c x[t-1] + sqrt(1 - phi_c^2) e[t]
 * with e the normals of xmca_surrogate rounded to the run dtype: stationary, unit variance, lag-1 autocorrelation phi_c.  The
 * recurrence runs in float64; phi_c = 0 leaves the white surrogate bit for bit.  Time is cut into segments that depend on
 * (T, N) only, so the surrogates do not depend on lanes, ranks or the device's load.
 *   xmca_lag1_autocorrelation  phi_out[c] (N float64, host) = sum_t (x[t]-m)(x[t+1]-m) / sum_t (x[t]-m)^2 of the columns of the
 *                              resident real plane of `side` (the handle's dtype; float64 after an extend='exp' / 'theta'
 *                              complexification), in float64, 0 for a constant column; the same bits on every call.
 *   xmca_rule_n_ar1            xmca_rule_n with the surrogates filtered: phi_left (Nx) / phi_right (Ny; NULL for one field) are
 *                              host arrays, uploaded once per call.  A value that is not finite or has |phi| >= 1 is
 *                              XMCA_ERR_INVALID, before anything is launched.
 *   xmca_rule_n_ar1_sharded    xmca_rule_n_sharded with those surrogates; phi must be the same on every rank.
 *   xmca_surrogate_ar1         (tests) the filtered, uncentred T x N field of (seed, run, side) in `dtype`, widened to float64.
 *   xmca_ar1_segments          (no device) the filter's segments at this shape: segment k covers the rows
 *                              [k length, min(T, (k + 1) length)), k < count. */
int xmca_lag1_autocorrelation(xmca_handle* h, int side, double* phi_out);
int xmca_rule_n_ar1(xmca_handle* h, int64_t T, int64_t Nx, int64_t Ny, int n_fields, const double* hilbert_col, int rotated,
                    int p, int power, double tol, int64_t run_begin, int64_t run_end, uint64_t seed, int dtype,
                    double* spectra_out, int* kept_out, int64_t n_out, const double* phi_left, const double* phi_right);
int xmca_rule_n_ar1_sharded(xmca_handle* h, xmca_comm* c, int64_t n_runs, int64_t T, int64_t Nx, int64_t Ny, int n_fields,
                            const double* hilbert_col, int rotated, int p, int power, double tol, uint64_t seed, int dtype,
                            double* spectra_out, int* kept_out, int64_t n_out, const double* phi_left, const double* phi_right);
int xmca_surrogate_ar1(xmca_handle* h, int64_t T, int64_t N, const double* phi, uint64_t seed, uint32_t run, uint32_t side, int dtype,
                       double* out);
int xmca_ar1_segments(int64_t T, int64_t N, int64_t* count_out, int64_t* length_out);

/* hipEvent stage timers of the calls since the last reset: names are written as a ';'-separated list.  Two
 * kernel-level entries follow the stages when the eigensolver ran: "jacobi_round_kernel_ms" (total duration of the
 * jacobi_fused_round_kernel launches, events around the rounds of every sweep) and "jacobi_round_kernel_launches"
 * (their number, in the ms array). */
int xmca_get_timings(xmca_handle* h, char* names, int names_len, double* ms, int max_n);

/* The kernels of the handle's last tridiagonal reduction by name (instantiation, column range of every launch of the chain), e.g.
 * "chain of 6 persistent launches: trd_resident_kernel<real,NC=24,RR=3,tagged> columns [0,512) -> ...": what `roofline.kernel`
 * of bench.py reports (ABI 9; until round 5 the bench synthesised the name from T).  Returns the length of the description. */
int xmca_get_reduction_info(xmca_handle* h, char* out, int out_len);
int xmca_reset_timings(xmca_handle* h);

/* Batched complex DFT used by the analytic-signal path (csrc/fft.h), host in / host out, for the parity tests:
 * out[b][k] = sum_t in[b][t] exp(sign 2 pi i k t / n), b < batch, k < n; planes of batch x n float64, in_im may be NULL.
 * Returns XMCA_ERR_UNSUPPORTED when n has a prime factor above 7 or exceeds 5120 (the solver then uses GEMMs). */
int xmca_fft(xmca_handle* h, const double* in_re, const double* in_im, int batch, int n, int sign, double* out_re, double* out_im);

/* Device memory kept by the handle.  The solver's temporaries come from a per-handle pool (hipFree waits for the whole
 * device): blocks are kept after a call, up to XMCA_POOL_LIMIT_GB (default 16) in total; an allocation failure empties every pool of the process first.
 * xmca_pool_bytes reports what is held right now (lanes of rule_n included), xmca_trim_pool gives it back to the driver. */
int xmca_pool_bytes(xmca_handle* h, int64_t* held_bytes);
int xmca_trim_pool(xmca_handle* h);

/* Kernel-level entry points used by the parity tests and the roofline leg of bench.py ------------------- */
/* C (M x N, float64, host) = alpha * op(A) op(B);  a_kfast: A(m,k) = A[m*lda + k] else A[k*lda + m];
 * b_nfast: B(k,n) = B[k*ldb + n] else B[n*ldb + k];  dtype of A and B; upper_only/mirror as in gemm.h. */
int xmca_gemm(xmca_handle* h, const void* A, int64_t lda, int a_kfast, const void* B, int64_t ldb, int b_nfast, double* C,
              int M, int N, int K, int dtype, double alpha, int upper_only, int mirror, int splits);
/* The same product with the epilogue options of gemm.h:  C = alpha * row_scale[m] * col_scale[n] * op(A) op(B) + beta * C.
 * C (host, M rows of ldc >= N elements, c_dtype XMCA_F32 / XMCA_F64) goes to the device as it is, is read only when
 * beta != 0, and comes back whole, the ldc - N padding elements of every row included; row_scale (M) and col_scale (N)
 * are host float64 arrays or NULL. */
int xmca_gemm_ex(xmca_handle* h, const void* A, int64_t lda, int a_kfast, const void* B, int64_t ldb, int b_nfast, void* C,
                 int64_t ldc, int c_dtype, int M, int N, int K, int dtype, double alpha, double beta, const double* row_scale,
                 const double* col_scale, int upper_only, int mirror, int splits);
/* Hermitian eigendecomposition of an n x n host matrix (interleaved complex when is_complex):
 * lam (n, descending) and Zh (n x n, row i = conj(u_i); NULL: eigenvalues only); info (4 ints): sweeps, tile, slots,
 * bit 0: Cholesky LR step taken, bit 1: solved by tridiagonalisation (csrc/tridiag.h; then no sweeps).  The device time of the
 * solve is recorded under "eigh_vectors" / "eigh_values" (xmca_get_timings). */
int xmca_eigh(xmca_handle* h, const double* A, int n, int is_complex, double* lam, double* Zh, int* info);
/* The same decomposition with the vectors of the n_lead (1 .. n) leading eigenvalues only, as the solver poses it for
 * solve(n_modes=k) (kernel tests only): lam gets all n values, Zh n_lead rows of n (row i = conj(u_i), descending).  On the
 * device the vector planes have n_lead + 1 rows of (n rounded up to 16) + 16 elements; the padding columns and the extra row
 * hold a sentinel before the solve.  info (6 ints): the four of xmca_eigh, the number of eigenvectors formed (n_lead or more
 * on the partial route, else n), and 1 when every sentinel word came back unchanged, 0 otherwise. */
int xmca_eigh_lead(xmca_handle* h, const double* A, int n, int is_complex, int n_lead, double* lam, double* Zh, int* info);
/* Host only, no handle, no device call: the number of eigenvectors the partial route forms for n_lead wanted ones given all n
 * eigenvalues in descending order (n: all of them), and in *rep_lead (may be NULL) whether bit-equal values among the leading
 * ones send the solve to the Jacobi sweeps - both exactly as the eigensolver decides them.  -1: bad arguments. */
int xmca_partial_count(const double* lam_desc, int n, int n_lead, int* rep_lead);
/* Blocked Cholesky of an n x n Hermitian host matrix (interleaved complex when is_complex): R (n x n, upper
 * triangular, row-major, same element layout) with R^H R = A + rel_shift * max(diag A) * I; *ok = 0 when a pivot was
 * not positive.  (The device routine behind the values-only two-field solve; exported for the kernel tests.) */
int xmca_cholesky(xmca_handle* h, const double* A, int n, int is_complex, double rel_shift, double* R, int* ok);
/* The same factorisation on the trailing block A[first:, first:] of a host buffer of n rows of lda >= n elements (interleaved
 * complex when is_complex), posed the way the one-sided solves pose it: base advanced by first * (lda + 1) elements, size
 * n - first, leading dimension lda.  The buffer goes to the device as it is and comes back whole in R (n x lda), so the
 * caller sees what was written outside the block.  (Kernel tests only.) */
int xmca_cholesky_ex(xmca_handle* h, const double* A, int n, int64_t lda, int first, int is_complex, double rel_shift, double* R, int* ok);
/* The skinny product behind the leading modes of a one-field solve (csrc/kernels.h lead_rows; kernel tests only), host in /
 * host out:  out[r*ldo + j] = scale[r] * sum_{k < K} A[r*lda + k] * B(k, j),  r < rows <= 16, j < n, with
 * B(k, j) = B[j*ldb + k] when b_kfast (B: n rows of ldb >= K) and B[k*ldb + j] otherwise (B: K rows of ldb >= n).  scale may be
 * NULL.  out (rows x ldo) goes to the device before the launch and comes back whole: padding returns as it went in.  *chunks
 * (may be NULL): into how many pieces the contraction was cut over the workgroups. */
int xmca_lead_rows(xmca_handle* h, const double* A, int64_t lda, const double* B, int64_t ldb, int b_kfast, int rows, int K, int n,
                   const double* scale, double* out, int64_t ldo, int* chunks);
/* The batched DFT of csrc/fft.h with every argument of fft_batch, host in / host out (kernel tests only):
 *   out[b*out_bs + k*out_es] = sa[k] sb[b] scale * sum_{t < n_in} x[b][t] exp(sign 2 pi i k t / n),  b < batch, k < n_keep,
 * x[b][t] = in[b*in_bs + t*in_es], or sin[t] * conj(in[...]) with conj_in (sin alone scales without conjugating).  in_im, sin
 * (n_in), sa (n_keep) and sb (batch) may be NULL.  in_re / in_im hold in_count elements, out_re / out_im out_count: the outputs
 * go to the device before the launch and come back whole, so untouched elements return as they went in.  1 <= n_in, n_keep <= n;
 * a request with an input or output index outside its buffer returns XMCA_ERR_INVALID before anything is launched. */
int xmca_fft_ex(xmca_handle* h, const double* in_re, const double* in_im, int64_t in_count, int64_t in_bs, int64_t in_es, int n_in,
                int conj_in, const double* sin, int batch, int n, int sign, double* out_re, double* out_im, int64_t out_count,
                int64_t out_bs, int64_t out_es, int n_keep, const double* sa, const double* sb, double scale);
/* The Sturm multisection behind every tridiagonal solve (csrc/tridiag.h trd_bisect_kernel; kernel tests only), host in / host out,
 * on a chosen symmetric tridiagonal matrix: d (n) its diagonal, e (n - 1; may be NULL for n = 1) its off-diagonal, float64 of any
 * magnitude.  d and e are multiplied by the power of two f a solve would apply - f * max(|d|, |e|) in [0.5, 1), f = 1 for a zero
 * matrix, the rule of trd_scale_kernel - and the kernel is launched as trd_eigenvalues launches it.  lam_desc: the n eigenvalues,
 * descending, in the caller's scale.  A non-finite entry returns XMCA_ERR_NUMERIC as a solve does; n < 1 or a NULL pointer
 * returns XMCA_ERR_INVALID before anything is launched. */
int xmca_tridiag_eigenvalues(xmca_handle* h, const double* d, const double* e, int n, double* lam_desc);
/* The twisted-factorisation vectors behind every tridiagonal solve (csrc/tridiag_vec.h trd_twisted_vectors; kernel tests only),
 * host in / host out: lam holds nev (1 .. n) eigenvalues of the matrix (d, e) above, ascending, in the scale of d and e - the
 * caller's, so nothing here depends on the Sturm kernel; the same f is applied to d, e and lam.  The kernel gets planes of n rows
 * of ldy >= nev elements: Y (n x ldy) goes to the device before the launch and comes back whole, column k the unit vector of
 * lam[k], the padding columns as they went in.  nev = n is the call of the full route, nev < n with the largest eigenvalues
 * that of the partial route.  nev < 1, nev > n, ldy < nev, n < 1 or a NULL pointer return XMCA_ERR_INVALID before anything is
 * launched; a non-finite entry XMCA_ERR_NUMERIC. */
int xmca_tridiag_vectors(xmca_handle* h, const double* d, const double* e, int n, const double* lam, int nev, double* Y, int64_t ldy);
/* Time `reps` Gram products G = X X^T of the resident field `side` with hipEvents on the library's stream;
 * avg_ms = mean duration of one product (all launches it needs), kernel_ms = mean duration of the MFMA
 * kernel launches alone, flops = useful flops of one product, T (T+1) N. */
int xmca_bench_gram(xmca_handle* h, int side, int reps, double* avg_ms, double* kernel_ms, double* flops);

/* Time `reps` launches of C = op(A) op(B) on device-resident pseudo-random operands (no host traffic):
 * avg_ms per product including the split-K reduction when one is used. */
int xmca_bench_gemm(xmca_handle* h, int M, int N, int K, int dtype, int a_kfast, int b_nfast, int upper_only, int splits,
                    int reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* XMCA_HIP_H */
