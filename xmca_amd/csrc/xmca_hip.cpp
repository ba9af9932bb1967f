// C ABI of libxmca_hip.so (see include/xmca_hip.h).  Compiled for gfx950 only.
#include <thread>
#include <exception>
#include "../../include/xmca_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>

#include "solver.h"
#include "comm.h"
#include "theta.h"
#include "boot_patterns.h"
#include "lag_gram.h"
#include "lag_project.h"
#include "lag_reconstruct.h"
#include "gap_fill.h"
#include "regress.h"
#include "time_filter.h"
#include "lead_lag.h"
#include "spectral.h"

using namespace xmca;

// The operator of a complexification X~ = X + i Op X along time (xmca_complexify / xmca_complexify_extended): the circulant
// Hilbert operator of scipy.signal.hilbert (first column, T values) or the operator of the fore/back-cast analytic signal of
// extend='exp' (xmca_amd/_hip.py extended_imag_parts: col3 of length 3T, hbar, U and W of T x r).  Host copies; the T x T matrix
// is assembled on the device when it is needed (build_operator).  extend='theta' (xmca_complexify_theta) is the extended operator
// of rank 0 plus B C: C the coefficients of the Theta fits of the columns (csrc/theta.h), B the images of their forecast basis.
struct ComplexOp {
  enum Kind { CIRCULANT, EXTENDED, THETA } kind = CIRCULANT;
  int64_t T = 0;
  int r = 0;
  int period = 0;                    // THETA: season length m
  std::vector<double> col, hbar, U, W;
  std::vector<double> B;             // THETA: T x 2 (THETA_HEAD + m), zero columns where a fit holds alpha, b0 and the level
  static ComplexOp circulant(const double* col, int64_t T) {
    ComplexOp op;
    op.T = T;
    op.col.assign(col, col + T);
    return op;
  }
  static ComplexOp extended(const double* col3, const double* hbar, const double* U, const double* W, int r, int64_t T) {
    ComplexOp op;
    op.kind = EXTENDED;
    op.T = T;
    op.r = r;
    op.col.assign(col3, col3 + 3 * T);
    op.hbar.assign(hbar, hbar + T);
    op.U.assign(U, U + T * r);
    op.W.assign(W, W + T * r);
    return op;
  }
  // B: T x 2 (2 + m) row-major, the forecast's columns (1, h, the m phases) and then the backcast's
  static ComplexOp theta(const double* col3, const double* hbar, const double* B, int period, int64_t T) {
    ComplexOp op = extended(col3, hbar, nullptr, nullptr, 0, T);
    op.kind = THETA;
    op.period = period;
    const int64_t kc = 2 + period, rows = ::xmca::theta_fit_rows(period);
    op.B.assign((size_t)(T * 2 * rows), 0.0);
    for (int64_t t = 0; t < T; ++t)
      for (int d = 0; d < 2; ++d)
        for (int64_t k = 0; k < kc; ++k) op.B[(t * 2 + d) * rows + (rows - kc) + k] = B[(t * 2 + d) * kc + k];
    return op;
  }
};

// What the handle holds in the fields' element type: the resident fields and the working copies of a bootstrap
// (xmca_bootstrap_begin).  xmca_handle::dtype says which of the two instances is live.
template <typename TI>
struct TypedState {
  FieldData<TI> f[2];
  DevBuf<TI> boot[2];
};

struct xmca_handle {
  ::xmca::DevPool pool;                   // first member: destroyed after every buffer below has gone back to it
  int device = 0;
  hipStream_t st = nullptr;
  std::vector<xmca_handle*> lanes;        // extra streams + workspaces for the concurrent surrogate lanes of rule_n
  std::string err;
  GemmWorkspace gws;
  EvdWorkspace ews;
  StageTimer tm;
  int dtype = -1;                         // XMCA_F32 / XMCA_F64: the live one of s32 / s64
  TypedState<float> s32;
  TypedState<double> s64;
  bool field_set[2] = {false, false};
  SolveResult res;
  bool solved = false;
  DeferredTail tail;                     // modes >= tail.head of `res` may still be in flight (join_tail)
  bool op_pending = false;               // complexify requested; carried out (or folded into the solve) lazily
  ComplexOp op;                          // ... with this operator
  RotationDevice rot;
  DevBuf<int> center_nan;          // scratch of center_columns
  DevBuf<double> center_sum;
  int64_t boot_T = 0, boot_N[2] = {0, 0};      // shape of the working copies of xmca_bootstrap_begin
  int boot_fields = 0;
};

// End of an entry point's try block: the error goes to `obj` (a handle or a communicator), its code is returned
#define XMCA_CATCH(obj)                                                \
  catch (const ::xmca::Error& e) {                                     \
    (obj)->err = e.what();                                             \
    (void)hipGetLastError();                                           \
    return e.code;                                                     \
  }                                                                    \
  catch (const std::exception& e) {                                    \
    (obj)->err = std::string("unexpected: ") + e.what();               \
    return XMCA_ERR_HIP;                                               \
  }                                                                    \
  return XMCA_OK;
// xmca_solve may return with the back-projection of the modes >= tail.head in flight on the tail's stream (solver.h
// DeferredTail).  Whoever reads those modes, changes what the tail reads (the fields) or starts the next solve waits here first;
// a failure of the tail surfaces here, and the result is then no result.
static void join_tail(xmca_handle* h) {
  if (!h->tail.pending) return;
  try {
    h->tm.add("backproject", h->tail.join());
  } catch (...) {
    h->solved = false;
    throw;
  }
}

// Start of an entry point's try block.  API_BEGIN joins the deferred tail: an entry point joins unless it says otherwise.
// API_BEGIN_NO_JOIN is for those that provably read no mode >= tail.head, no field and nothing the tail's stream touches.
#define API_BEGIN_NO_JOIN(h)                                           \
  if (!(h)) return XMCA_ERR_INVALID;                                   \
  try {                                                                \
    ::xmca::PoolScope _pool_scope(&(h)->pool);                         \
    XMCA_HIP(hipSetDevice((h)->device));
#define API_BEGIN(h)                                                   \
  API_BEGIN_NO_JOIN(h)                                                 \
    join_tail(h);
#define API_END(h) } XMCA_CATCH(h)

extern "C" {

const char* xmca_version(void) { return "xmca_amd 0.2.0 (gfx950)"; }
int xmca_abi_version(void) { return XMCA_ABI_VERSION; }

int xmca_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

int xmca_create(int device, xmca_handle** out) {
  if (!out) return XMCA_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); return XMCA_ERR_HIP; }
  if (hipSetDevice(device) != hipSuccess) return XMCA_ERR_HIP;
  // XMCA_BLOCKING_SYNC=1: the host threads of this process sleep on an interrupt while they wait for the device instead of
  // spinning (measured: 1.4 host cores per process while the GPU works -> 0.5; +0.3 ms per 14 ms eigensolve).  For several
  // ranks / surrogate lanes sharing few host cores: a cgroup CPU quota exhausted by spinning threads stalls every thread of
  // the container for the rest of the period ("Host threads"); bench.py sets it for runs of several ranks.
  // Default (variable unset): blocking whenever the launcher says this process is one of several ranks of a node
  // (LOCAL_WORLD_SIZE / WORLD_SIZE > 1 - torchrun, mpirun wrappers): 8 spinning ranks need 20 host cores where a GPU box grants 16
  // (profiles/r05_host_budget.json).  XMCA_BLOCKING_SYNC=0 keeps the spinning waits.
  {
    const char* e = std::getenv("XMCA_BLOCKING_SYNC");
    bool blocking = e && e[0] == '1';
    if (!e || !e[0]) {
      for (const char* name : {"LOCAL_WORLD_SIZE", "WORLD_SIZE"}) {
        const char* w = std::getenv(name);
        if (w && std::atoi(w) > 1) blocking = true;
      }
    }
    if (blocking) { (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync); (void)hipGetLastError(); }
  }
  xmca_handle* h = new xmca_handle();
  h->device = device;
  if (hipStreamCreate(&h->st) != hipSuccess) { delete h; return XMCA_ERR_HIP; }
  h->tm.st = h->st;
  *out = h;
  return XMCA_OK;
}

void xmca_destroy(xmca_handle* h) {
  if (!h) return;
  for (xmca_handle* lane : h->lanes) xmca_destroy(lane);
  h->lanes.clear();
  (void)hipSetDevice(h->device);
  try { join_tail(h); } catch (...) {}
  (void)hipStreamSynchronize(h->st);
  try { h->tm.reset(); } catch (...) {}
  (void)hipStreamDestroy(h->st);
  delete h;
}

const char* xmca_last_error(xmca_handle* h) { return h ? h->err.c_str() : "null handle"; }

}  // extern "C"

namespace {

template <typename TI>
TypedState<TI>& typed(xmca_handle* h) {
  if constexpr (std::is_same<TI, float>::value) return h->s32;
  else return h->s64;
}

// The one dtype dispatch: f(float{}) or f(double{}) for a run-time XMCA_F32 / XMCA_F64 code; the callee takes its element
// type from the tag, with_dtype(code, [&](auto t) { foo<decltype(t)>(...); })
template <typename F>
void with_dtype(int code, F&& f) {
  if (code == XMCA_F32) f(float{});
  else f(double{});
}

// number of time steps of the resident fields
int64_t resident_T(xmca_handle* h) {
  int64_t T = 0;
  with_dtype(h->dtype, [&](auto t) { T = typed<decltype(t)>(h).f[0].T; });
  return T;
}

// number of columns of the resident field of `side`
int64_t resident_N(xmca_handle* h, int side) {
  int64_t N = 0;
  with_dtype(h->dtype, [&](auto t) { N = typed<decltype(t)>(h).f[side].N; });
  return N;
}

// ---- argument checks shared by the entry points (`what`: the entry point's prefix of the message) ---------------------------
void check_side(const char* what, int side) {
  XMCA_CHECK(side == 0 || side == 1, XMCA_ERR_INVALID, std::string(what) + ": side must be 0 or 1");
}

// a caller's device pointer (xmca_set_field_strided, the XMCA_DEVICE outputs): device memory of the handle's GPU
void check_device_pointer(xmca_handle* h, const char* what, const void* p) {
  hipPointerAttribute_t a;
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) (void)hipGetLastError();
  XMCA_CHECK(e == hipSuccess && a.type == hipMemoryTypeDevice && a.device == h->device, XMCA_ERR_INVALID,
             std::string(what) + ": not a pointer to memory of the handle's device");
}

// the memory space of an output: XMCA_HOST, or XMCA_DEVICE with a pointer the handle's GPU can write
void check_out_location(xmca_handle* h, const char* what, int location, const void* out) {
  XMCA_CHECK(location == XMCA_HOST || location == XMCA_DEVICE, XMCA_ERR_INVALID, std::string(what) + ": the location must be XMCA_HOST or XMCA_DEVICE");
  if (location == XMCA_DEVICE) check_device_pointer(h, what, out);
}

// rotation of every replicate (xmca_rule_n, xmca_bootstrap_runs*); `detail`: the entry point's own wording of the requirement
void check_rotation_args(const char* what, const char* detail, int rotated, int p, int power) {
  XMCA_CHECK(!rotated || (p >= 2 && power >= 1), XMCA_ERR_INVALID, std::string(what) + ": " + detail);
}

// the parts of the extended operator (xmca_complexify_extended, xmca_bootstrap_runs_extended)
void check_extended_parts(const char* what, const double* col3, const double* hbar, const double* U, const double* W, int rank) {
  XMCA_CHECK(col3 && hbar && rank >= 0 && rank <= 16 && (rank == 0 || (U && W)), XMCA_ERR_INVALID,
             std::string(what) + ": need col3, hbar and T x rank U, W (rank <= 16)");
}

// ... and the bound on the T of its T x T assembly (46340^2 < 2^31)
void check_operator_size(const char* what, int64_t T) {
  XMCA_CHECK(T <= 46340, XMCA_ERR_UNSUPPORTED, std::string(what) + ": T x T operator too large");
}

void check_bootstrap_runs(const double* spectra_out, const int* kept_out, int64_t n_out, int64_t n_runs, int rotated,
                          int p, int power) {
  XMCA_CHECK(spectra_out && kept_out && n_out >= 1 && n_runs >= 0, XMCA_ERR_INVALID, "bootstrap: output buffers missing");
  check_rotation_args("bootstrap", "rotation needs n_rot >= 2 and power >= 1", rotated, p, power);
}

// the kept columns of a masked output: N of N_full <= max_full columns, keep_idx (NULL: all of them, N_full == N) their strictly
// increasing indices in [0, N_full)
void check_kept_columns(const char* what, const int64_t* keep_idx, int64_t N, int64_t N_full, int64_t max_full) {
  const std::string w(what);
  XMCA_CHECK(N_full >= N && N_full <= max_full && (keep_idx || N_full == N), XMCA_ERR_INVALID,
             w + ": N_full must be the " + std::to_string(N) + " kept columns, or more with keep_idx");
  for (int64_t c = 0; keep_idx && c < N; ++c)
    XMCA_CHECK(keep_idx[c] >= 0 && keep_idx[c] < N_full && (c == 0 || keep_idx[c] > keep_idx[c - 1]), XMCA_ERR_INVALID,
               w + ": keep_idx must be increasing indices below N_full, one per kept column");
}

// the resident field of side 0 and the embedding of the lag entries: a real field, embedding and tau >= 1, T' >= min_window
int64_t check_lag_embedding(xmca_handle* h, const char* what, int embedding, int tau, int64_t min_window) {
  const std::string w(what);
  XMCA_CHECK(h->field_set[0], XMCA_ERR_STATE, w + ": no field set");
  XMCA_CHECK(embedding >= 1 && tau >= 1, XMCA_ERR_INVALID, w + ": embedding and tau must be at least 1");
  bool has_im = false;
  with_dtype(h->dtype, [&](auto t) { has_im = typed<decltype(t)>(h).f[0].has_im; });
  XMCA_CHECK(!has_im && !h->op_pending, XMCA_ERR_INVALID, w + ": the resident field is complex (real fields only)");
  const int64_t T = resident_T(h);
  check_operator_size(what, T);
  const int64_t np = T - (int64_t)(embedding - 1) * tau;
  XMCA_CHECK(np >= min_window, XMCA_ERR_INVALID, w + ": T - (embedding - 1) * tau must be at least " + std::to_string(min_window));
  return np;
}

// the plane of the gap entries: dtype, T x N within the eigensolver's and the kernels' index ranges
void check_gap_plane(const char* what, int64_t T, int64_t N, int dtype) {
  const std::string w(what);
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, w + ": dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(T >= 1 && N >= 1, XMCA_ERR_INVALID, w + ": the field must have at least one row and one column");
  check_operator_size(what, T);
  XMCA_CHECK(N < ((int64_t)1 << 31) && T * N < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED, w + ": field too large");
}

// ---- host arrays <-> device planes --------------------------------------------------------------------------------------------
// A host float64 array of n elements, interleaved complex when `cplx`, as device planes r / i (nullptr: real) of TP.  It is
// uploaded into `stage` and split (complex) or converted (real) from there; convert_real = false (TP = double only) uses a real
// array where it was uploaded, without a pass.  `stage` must not go back to the pool before the stream has passed the split /
// conversion: the caller keeps the struct alive that long or synchronises first.
template <typename TP>
struct HostPlanes {
  DevBuf<double> stage;
  DevBuf<TP> re, im;
  const TP* r = nullptr;
  const TP* i = nullptr;
};

template <typename TP>
void upload_planes(xmca_handle* h, const double* host, size_t n, bool cplx, HostPlanes<TP>& p, bool convert_real = true) {
  const size_t n_host = n * (cplx ? 2 : 1);
  XMCA_HIP(hipMemcpyAsync(p.stage.ensure(n_host), host, sizeof(double) * n_host, hipMemcpyHostToDevice, h->st));
  p.i = nullptr;
  if (cplx) {
    hipLaunchKernelGGL((split_complex_kernel<double, TP>), ew_grid((int64_t)n), dim3(EW_BLOCK), 0, h->st, p.stage.get(), p.re.ensure(n),
                       p.im.ensure(n), (int64_t)n);
    p.r = p.re.get();
    p.i = p.im.get();
  } else if (convert_real) {
    hipLaunchKernelGGL((convert_kernel<double, TP>), ew_grid((int64_t)n), dim3(EW_BLOCK), 0, h->st, p.stage.get(), p.re.ensure(n), (int64_t)n);
    p.r = p.re.get();
  } else if constexpr (std::is_same<TP, double>::value) {
    p.r = p.stage.get();
  }
  XMCA_HIP(hipGetLastError());
}

// rows x cols device planes (row stride ld; im == nullptr: real) -> host array of TO, interleaved when complex, through `packed`
// (rows * cols * (im ? 2 : 1) elements).  The caller synchronises the stream before `packed` goes back to the pool.
template <typename TO>
void pack_download(xmca_handle* h, const double* re, const double* im, int64_t ld, int rows, int cols, TO* packed, void* host) {
  hipLaunchKernelGGL((pack_rows_kernel<TO>), ew_grid((int64_t)rows * cols), dim3(EW_BLOCK), 0, h->st, re, im, ld, rows, cols, packed, 0);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(host, packed, sizeof(TO) * (size_t)rows * cols * (im ? 2 : 1), hipMemcpyDeviceToHost, h->st));
}

// The inverse of keep_idx on the device: entry n of N_full is the kept column that full column n is, or -1.  Returns its device
// pointer, or null without keep_idx (every column kept).
const int64_t* upload_inverse_map(xmca_handle* h, const int64_t* keep_idx, int64_t N, int64_t N_full, DevBuf<int64_t>& dev) {
  if (!keep_idx) return nullptr;
  std::vector<int64_t> inv((size_t)N_full, -1);
  for (int64_t c = 0; c < N; ++c) inv[(size_t)keep_idx[c]] = c;
  XMCA_HIP(hipMemcpyAsync(dev.ensure((size_t)N_full), inv.data(), sizeof(int64_t) * N_full, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));      // (inv is a host temporary)
  return dev.get();
}

template <typename TI>
void set_field_impl(xmca_handle* h, int side, const void* re, const void* im, int64_t T, int64_t N, int location) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  const size_t n = (size_t)T * N;
  f.T = T; f.N = N;
  f.has_im = im != nullptr;
  f.ext_re = nullptr; f.ext_im = nullptr;
  if (location == XMCA_DEVICE) {
    f.ext_re = static_cast<const TI*>(re);
    f.ext_im = static_cast<const TI*>(im);
  } else {
    XMCA_HIP(hipMemcpyAsync(f.re.ensure(n), re, n * sizeof(TI), hipMemcpyHostToDevice, h->st));
    if (im) XMCA_HIP(hipMemcpyAsync(f.im.ensure(n), im, n * sizeof(TI), hipMemcpyHostToDevice, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
  }
}

// T x T circulant Hilbert operator in the field's element type, from its first column (host)
template <typename TI>
void build_hilbert(xmca_handle* h, const double* col_host, int64_t T, DevBuf<TI>& ht) {
  DevBuf<double> col;
  XMCA_HIP(hipMemcpyAsync(col.ensure((size_t)T), col_host, sizeof(double) * T, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL((circulant_kernel<TI>), ew_grid(T * T), dim3(EW_BLOCK), 0, h->st, col.get(), (int)T, ht.ensure((size_t)T * T));
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// T x T operator of `op` in the field's element type: the circulant Hilbert operator, or the extended one (row means removed)
template <typename TI>
void build_operator(xmca_handle* h, const ComplexOp& op, DevBuf<TI>& g) {
  if (op.kind == ComplexOp::CIRCULANT) {
    build_hilbert<TI>(h, op.col.data(), op.T, g);
    return;
  }
  const int64_t T = op.T;
  XMCA_CHECK((int64_t)op.col.size() == 3 * T && (int64_t)op.hbar.size() == T && (int64_t)op.U.size() == T * op.r &&
                 (int64_t)op.W.size() == T * op.r,
             XMCA_ERR_STATE, "extended operator: inconsistent parts");
  DevBuf<double> col3, hbar, U, W;
  XMCA_HIP(hipMemcpyAsync(col3.ensure((size_t)(3 * T)), op.col.data(), sizeof(double) * 3 * T, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(hbar.ensure((size_t)T), op.hbar.data(), sizeof(double) * T, hipMemcpyHostToDevice, h->st));
  U.ensure((size_t)(T * op.r) + 1);
  W.ensure((size_t)(T * op.r) + 1);
  if (op.r > 0) {                 // (rank 0: the operator of extend='theta', nothing to copy)
    XMCA_HIP(hipMemcpyAsync(U.get(), op.U.data(), sizeof(double) * T * op.r, hipMemcpyHostToDevice, h->st));
    XMCA_HIP(hipMemcpyAsync(W.get(), op.W.data(), sizeof(double) * T * op.r, hipMemcpyHostToDevice, h->st));
  }
  hipLaunchKernelGGL((extended_operator_kernel<TI>), ew_grid(T * T), dim3(EW_BLOCK), 0, h->st, col3.get(), hbar.get(), U.get(), W.get(),
                     op.r, (int)T, g.ensure((size_t)T * T));
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// "Apply this operator to a centred real field", stated once (complexify_impl, ReplicateRunner::run): the imaginary plane of `f`
// becomes g X, g the T x T device operator of build_operator, plus B C when `bdev` is given (extend='theta': bdev T x kb, `fit`
// the kb x N Theta fits of X, theta_fit).  Queued on the handle's stream.
template <typename TI>
void apply_operator(xmca_handle* h, const TI* g, const double* bdev, const double* fit, int kb, FieldData<TI>& f) {
  const int64_t T = f.T, N = f.N;
  GemmOpts o;   // X_im = Ht X (or G X)   (T x T) (T x N)
  TI* dst = f.im.ensure((size_t)T * N);
  gemm<TI, TI>(h->st, h->gws, g, T, f.r(), N, dst, N, (int)T, (int)N, (int)T, o);
  if constexpr (std::is_same<TI, double>::value) {
    if (bdev) {   // X_im += B C   (T x kb) (kb x N)
      GemmOpts acc;
      acc.beta = 1.0;
      gemm<double, double>(h->st, h->gws, bdev, kb, fit, N, dst, N, (int)T, (int)N, kb, acc);
    }
  }
  f.has_im = true;
  f.ext_im = nullptr;
}

template <typename TI>
void complexify_impl(xmca_handle* h, const ComplexOp& op) {
  FieldData<TI>* f = typed<TI>(h).f;
  const int64_t T = f[0].T;
  XMCA_CHECK(op.T == T, XMCA_ERR_STATE, "complexify: the operator was made for another number of time steps");
  DevBuf<TI> htb;
  build_operator<TI>(h, op, htb);
  struct { const TI* r; } ht{htb.get()};
  // extend='theta': the fits of every column first, C (2 (THETA_HEAD + m) x N per field); they stay on the device
  const bool theta = op.kind == ComplexOp::THETA;
  DevBuf<double> fit[2], bdev;
  const int kb = theta ? (int)(2 * theta_fit_rows(op.period)) : 0;
  if (theta) {
    XMCA_CHECK((std::is_same<TI, double>::value), XMCA_ERR_STATE, "complexify_theta: the fields must be float64");
    XMCA_CHECK((int64_t)op.B.size() == T * kb, XMCA_ERR_STATE, "complexify_theta: inconsistent parts");
    XMCA_HIP(hipMemcpyAsync(bdev.ensure(op.B.size()), op.B.data(), sizeof(double) * op.B.size(), hipMemcpyHostToDevice, h->st));
    h->tm.begin("theta_fit");
    if constexpr (std::is_same<TI, double>::value) {
      for (int s = 0; s < 2; ++s)
        if (h->field_set[s]) theta_fit(h->st, f[s].r(), T, f[s].N, op.period, fit[s].ensure((size_t)kb * f[s].N));
    }
    h->tm.end();
  }
  h->tm.begin(op.kind == ComplexOp::CIRCULANT ? "hilbert" : "hilbert_extended");
  for (int s = 0; s < 2; ++s)
    if (h->field_set[s]) apply_operator<TI>(h, ht.r, theta ? bdev.get() : nullptr, fit[s].get(), kb, f[s]);
  h->tm.end();
  XMCA_HIP(hipStreamSynchronize(h->st));
}

template <typename TI>
void solve_impl(xmca_handle* h, int n_fields, int64_t n_vec) {
  FieldData<TI>* f = typed<TI>(h).f;
  if (n_vec > 0) {
    // A buffer only grows: the planes of an earlier, larger result on this handle would stay behind a result of n_vec modes.
    // They go back to the pool (xmca_trim_pool frees them) and the solve takes blocks of the size it needs.
    for (int s = 0; s < 2; ++s) { h->res.Vt[s].re.release(); h->res.Vt[s].im.release(); h->res.Vt32[s].release(); }
  }
  if (h->op_pending) {
    if (Solver<TI>::analytic_route(h->op.kind == ComplexOp::CIRCULANT, f[0].T, f[0].N, n_fields == 2 ? f[1].N : 0, n_fields,
                                   f[0].has_im || (n_fields == 2 && f[1].has_im))) {
      Solver<TI> s(h->st, h->gws, h->ews, h->tm);
      s.partial_vectors = true;
      s.solve_analytic(f, n_fields, (int)n_vec, h->res);
      return;
    }
    complexify_impl<TI>(h, h->op);
    h->op_pending = false;
  }
  const bool cplx = f[0].has_im;
  if (n_fields == 2) XMCA_CHECK(f[1].has_im == cplx, XMCA_ERR_INVALID, "solve: both fields must be real or both complex");
  Solver<TI> s(h->st, h->gws, h->ews, h->tm);
  s.f32_vectors = true;          // (only the one-field dual route of a real float32 field uses it)
  s.partial_vectors = true;      // (one field, n_vec > 0: no more eigenvectors are formed than modes are back-projected)
  if (n_fields == 1) {           // ... and only it may leave the tail of its back-projection in flight
    h->tail.count_call();
    s.defer = &h->tail;
  }
  s.solve(f, n_fields, cplx, (int)n_vec, h->res);
}

template <typename TO>
void get_vectors_impl(xmca_handle* h, int side, void* out, int64_t m) {
  const SolveResult& r = h->res;
  const int64_t N = r.ldv[side];
  const bool cplx = r.cplx;
  const size_t n_out = (size_t)m * N * (cplx ? 2 : 1);
  if (r.vt_f32[side]) {              // float32-resident vectors (real, dense m x N): straight out, or widened
    if constexpr (std::is_same<TO, float>::value) {
      XMCA_HIP(hipMemcpyAsync(out, r.Vt32[side].get(), n_out * sizeof(float), hipMemcpyDeviceToHost, h->st));
    } else {
      DevBuf<TO> wide;
      hipLaunchKernelGGL((convert_kernel<float, TO>), ew_grid((int64_t)n_out), dim3(EW_BLOCK), 0, h->st, r.Vt32[side].get(), wide.ensure(n_out),
                         (int64_t)n_out);
      XMCA_HIP(hipGetLastError());
      XMCA_HIP(hipMemcpyAsync(out, wide.get(), n_out * sizeof(TO), hipMemcpyDeviceToHost, h->st));
    }
    XMCA_HIP(hipStreamSynchronize(h->st));
    return;
  }
  DevBuf<TO> tmp;
  // (the caller has joined unless m <= tail.head; on the lead route those modes are in a buffer of their own until the join)
  const double* lead = h->tail.lead_modes();
  pack_download<TO>(h, lead ? lead : r.Vt[side].r(), r.Vt[side].i(cplx), N, (int)m, (int)N, tmp.ensure(n_out), out);
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// EOFs of `side` in the reference's final layout (see xmca_get_eofs): N x q, mixed on the device from the resident mode-major vectors
// ... into `tmp` on the device (N x q, interleaved when the model or W is complex); `w` holds the uploaded W until the caller has
// synchronised the stream
template <typename TO>
void eofs_compact(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, bool w_cplx, HostPlanes<double>& w, DevBuf<TO>& tmp) {
  const SolveResult& r = h->res;
  const int64_t N = r.ldv[side];
  const bool v_cplx = r.cplx, o_cplx = v_cplx || (W && w_cplx);
  const size_t n_out = (size_t)N * q * (o_cplx ? 2 : 1);
  tmp.ensure(n_out);
  if (W) {
    upload_planes<double>(h, W, (size_t)m * q, w_cplx, w, false);
    const dim3 grid((unsigned)ceil_div(N, 256));
    if (r.vt_f32[side])
      hipLaunchKernelGGL((eof_mix_kernel<float, TO>), grid, dim3(256), 0, h->st, r.Vt32[side].get(), (const float*)nullptr, N, N, (int)m, (int)q, w.r, w.i, tmp.get());
    else
      hipLaunchKernelGGL((eof_mix_kernel<double, TO>), grid, dim3(256), 0, h->st, r.Vt[side].r(), r.Vt[side].i(v_cplx), N, N, (int)m, (int)q, w.r, w.i, tmp.get());
  } else {
    const dim3 grid((unsigned)ceil_div(N, 32), (unsigned)ceil_div(q, 32));
    if (r.vt_f32[side])
      hipLaunchKernelGGL((eof_transpose_kernel<float, TO>), grid, dim3(256), 0, h->st, r.Vt32[side].get(), (const float*)nullptr, N, N, (int)q, tmp.get());
    else
      hipLaunchKernelGGL((eof_transpose_kernel<double, TO>), grid, dim3(256), 0, h->st, r.Vt[side].r(), r.Vt[side].i(v_cplx), N, N, (int)q, tmp.get());
  }
  XMCA_HIP(hipGetLastError());
}

template <typename TO>
void get_eofs_impl(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, bool w_cplx, void* out) {
  const bool o_cplx = h->res.cplx || (W && w_cplx);
  const size_t n_out = (size_t)h->res.ldv[side] * q * (o_cplx ? 2 : 1);
  DevBuf<TO> tmp;
  HostPlanes<double> w;
  eofs_compact<TO>(h, side, W, m, q, w_cplx, w, tmp);
  XMCA_HIP(hipMemcpyAsync(out, tmp.get(), n_out * sizeof(TO), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// Spatial maps of `side` in their final N_full x q layout (see xmca_get_maps): the compact EOFs as above, the divisors of the
// columns (partials per workgroup, merged in a fixed order), then one pass that applies factor, divisor, amplitude / phase and the
// mask.  The compact values are read twice, the output is written once.
template <typename TO>
void get_maps_impl(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, bool w_cplx, const double* col_factor, bool f_cplx,
                   const int64_t* keep_idx, int64_t N_full, int kind, int scaling, void* out, double* stat_out, bool out_dev) {
  const int64_t N = h->res.ldv[side];
  const bool c_cplx = h->res.cplx || (W && w_cplx);
  const bool o_cplx = kind == MAP_EOF && (c_cplx || (col_factor && f_cplx));
  DevBuf<double> tmp, part, div;      // (the compact values stay float64: rounded once, at the end)
  DevBuf<TO> fin;
  DevBuf<int64_t> row_of;
  HostPlanes<double> w, f;
  eofs_compact<double>(h, side, W, m, q, w_cplx, w, tmp);
  if (col_factor) upload_planes<double>(h, col_factor, (size_t)q, f_cplx, f, false);
  const int64_t* rows = upload_inverse_map(h, keep_idx, N, N_full, row_of);
  h->tm.begin("maps");
  if (scaling != XMCA_SCALE_NONE) {
    const int blocks = (int)std::min<int64_t>(ceil_div(N, (int64_t)256), MAP_STAT_BLOCKS);
    const int np = scaling == XMCA_SCALE_STD ? 3 : 1;
    part.ensure((size_t)blocks * q * np);
    div.ensure((size_t)q);
    const dim3 fgrid((unsigned)ceil_div(q, (int64_t)256));
    auto stats = [&](auto stat) {
      constexpr int STAT = decltype(stat)::value;
      hipLaunchKernelGGL((map_column_partials_kernel<STAT>), dim3((unsigned)blocks), dim3(256), 0, h->st, tmp.get(), (int)c_cplx, N, (int)q,
                         f.r, f.i, part.get());
      hipLaunchKernelGGL((map_column_finish_kernel<STAT>), fgrid, dim3(256), 0, h->st, part.get(), blocks, (int)q, div.get());
    };
    if (scaling == XMCA_SCALE_STD) stats(std::integral_constant<int, STAT_STD>{});
    else if (kind == MAP_AMPLITUDE) stats(std::integral_constant<int, STAT_MAX_AMP>{});
    else stats(std::integral_constant<int, STAT_MAX_RE>{});
    XMCA_HIP(hipGetLastError());
  }
  const size_t total = (size_t)N_full * q;
  hipLaunchKernelGGL((map_finish_kernel<TO>), ew_grid((int64_t)total), dim3(EW_BLOCK), 0, h->st, tmp.get(), (int)c_cplx,
                     rows, N_full, (int)q, f.r, f.i, scaling != XMCA_SCALE_NONE ? div.get() : nullptr, kind,
                     (int)o_cplx, out_dev ? static_cast<TO*>(out) : fin.ensure(total * (o_cplx ? 2 : 1)));     // (a device destination is final)
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  if (stat_out && scaling != XMCA_SCALE_NONE)
    XMCA_HIP(hipMemcpyAsync(stat_out, div.get(), sizeof(double) * q, hipMemcpyDeviceToHost, h->st));
  if (!out_dev) XMCA_HIP(hipMemcpyAsync(out, fin.get(), sizeof(TO) * total * (o_cplx ? 2 : 1), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// U = X~ V on the resident field of `side` (see xmca_project)
template <typename TI>
void project_impl(xmca_handle* h, int side, const void* V, int64_t N, int64_t m, bool v_cplx, void* U_out, int* out_cplx) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  XMCA_CHECK(f.N == N, XMCA_ERR_INVALID, "project: V has " + std::to_string(N) + " rows, the field has " + std::to_string(f.N) + " columns");
  const int64_t T = f.T;
  if (h->op_pending && h->op.kind != ComplexOp::CIRCULANT) {    // no implicit form: the imaginary planes G X (+ B C) are formed first
    complexify_impl<TI>(h, h->op);
    h->op_pending = false;
  }
  const bool analytic = !f.has_im && h->op_pending;            // imaginary plane implicit: X~ = X + i Ht X
  const bool f_cplx = f.has_im || analytic, cplx = f_cplx || v_cplx;
  // V -> planes in the field's element type (N x m, ld = m): from the host, or (V == NULL) the first m resident vectors of the last
  // solve transposed on the device - the same values as fetched, widened to float64 and uploaded again
  const size_t nv = (size_t)N * m;
  HostPlanes<TI> vp;
  DevBuf<TI>& vr = vp.re;        // (the resident branch fills the same planes)
  DevBuf<TI>& vi = vp.im;
  DevBuf<TI> vt;
  if (V) {
    upload_planes<TI>(h, static_cast<const double*>(V), nv, v_cplx, vp);
  } else {
    const SolveResult& r = h->res;
    v_cplx = r.cplx;
    const dim3 grid((unsigned)ceil_div(N, 32), (unsigned)ceil_div(m, 32));
    if (r.vt_f32[side]) {
      hipLaunchKernelGGL((eof_transpose_kernel<float, TI>), grid, dim3(256), 0, h->st, r.Vt32[side].get(), (const float*)nullptr, r.ldv[side], N,
                         (int)m, vr.ensure(nv));
    } else if (!v_cplx) {
      hipLaunchKernelGGL((eof_transpose_kernel<double, TI>), grid, dim3(256), 0, h->st, r.Vt[side].r(), (const double*)nullptr, r.ldv[side], N,
                         (int)m, vr.ensure(nv));
    } else {
      hipLaunchKernelGGL((eof_transpose_kernel<double, TI>), grid, dim3(256), 0, h->st, r.Vt[side].r(), r.Vt[side].i(true), r.ldv[side], N,
                         (int)m, vt.ensure(2 * nv));
      XMCA_HIP(hipGetLastError());
      hipLaunchKernelGGL((split_complex_kernel<TI, TI>), ew_grid((int64_t)nv), dim3(EW_BLOCK), 0, h->st, vt.get(), vr.ensure(nv), vi.ensure(nv),
                         (int64_t)nv);
    }
  }
  XMCA_HIP(hipGetLastError());
  h->tm.begin("project");
  DevBuf<double> wr, wi, ur, ui;
  const size_t nu = (size_t)T * m;
  wr.ensure(nu);
  if (cplx) wi.ensure(nu);
  // W = X V on the stored planes (complex x complex through cgemm; a missing plane is a zero plane)
  if (f.has_im || v_cplx) {
    if (f.has_im && v_cplx) {
      cgemm<TI>(h->st, h->gws, f.r(), f.i(), f.N, true, false, vr.get(), vi.get(), m, true, false, wr.get(), wi.get(), m, (int)T,
                (int)m, (int)N, 1.0, nullptr, nullptr, false);
    } else if (f.has_im) {      // complex field, real V
      GemmOpts o;
      gemm<TI, double>(h->st, h->gws, f.r(), f.N, vr.get(), m, wr.get(), m, (int)T, (int)m, (int)N, o);
      gemm<TI, double>(h->st, h->gws, f.i(), f.N, vr.get(), m, wi.get(), m, (int)T, (int)m, (int)N, o);
    } else {                    // real field plane, complex V
      GemmOpts o;
      gemm<TI, double>(h->st, h->gws, f.r(), f.N, vr.get(), m, wr.get(), m, (int)T, (int)m, (int)N, o);
      gemm<TI, double>(h->st, h->gws, f.r(), f.N, vi.get(), m, wi.get(), m, (int)T, (int)m, (int)N, o);
    }
  } else {
    GemmOpts o;
    gemm<TI, double>(h->st, h->gws, f.r(), f.N, vr.get(), m, wr.get(), m, (int)T, (int)m, (int)N, o);
    if (cplx) XMCA_HIP(hipMemsetAsync(wi.get(), 0, sizeof(double) * nu, h->st));
  }
  const double* out_r = wr.get();
  const double* out_i = cplx ? wi.get() : nullptr;
  DevBuf<double> ht;
  if (analytic) {
    // U = W + i Ht W:  Ur = Wr - Ht Wi,  Ui = Wi + Ht Wr
    XMCA_CHECK(h->op.kind == ComplexOp::CIRCULANT && h->op.T == T, XMCA_ERR_STATE, "project: the Hilbert column of the model is missing");
    build_hilbert<double>(h, h->op.col.data(), T, ht);
    XMCA_HIP(hipMemcpyAsync(ur.ensure(nu), wr.get(), sizeof(double) * nu, hipMemcpyDeviceToDevice, h->st));
    XMCA_HIP(hipMemcpyAsync(ui.ensure(nu), wi.get(), sizeof(double) * nu, hipMemcpyDeviceToDevice, h->st));
    GemmOpts o;
    o.beta = 1.0;
    o.alpha = -1.0;
    gemm<double, double>(h->st, h->gws, ht.get(), T, wi.get(), m, ur.get(), m, (int)T, (int)m, (int)T, o);
    o.alpha = 1.0;
    gemm<double, double>(h->st, h->gws, ht.get(), T, wr.get(), m, ui.get(), m, (int)T, (int)m, (int)T, o);
    out_r = ur.get();
    out_i = ui.get();
  }
  h->tm.end();
  DevBuf<double> packed;
  pack_download<double>(h, out_r, out_i, m, (int)T, (int)m, packed.ensure(nu * (cplx ? 2 : 1)), U_out);
  XMCA_HIP(hipStreamSynchronize(h->st));
  *out_cplx = cplx ? 1 : 0;
}

// ---- forward / inverse transform of new data (xmca_predict, xmca_reconstruct) -------------------------------------------------
// Rows of new data (predict) or of a reconstruction (reconstruct) are processed in blocks of at most this many bytes of T x N
// data, so that neither a long new record nor a long reconstruction has to be resident at once.
constexpr int64_t TRANSFORM_BLOCK_BYTES = (int64_t)128 << 20;

int64_t transform_rows(int64_t T, int64_t row_bytes) {
  const int64_t rows = TRANSFORM_BLOCK_BYTES / std::max<int64_t>(row_bytes, 1);
  return std::max<int64_t>(1, std::min<int64_t>(T, rows));
}

// The m leading vectors of `side` as one operand of a product over grid points, in the product's element type TP: the resident
// mode-major planes of the last solve (V == NULL; element (n, j) at j * ld + n) or a host N x m array uploaded as float64 planes
// (element (n, j) at n * m + j).
template <typename TP>
struct VecOperand {
  const TP* r = nullptr;
  const TP* i = nullptr;        // nullptr: real vectors
  int64_t ld = 0;
  bool mode_major = true;
  HostPlanes<TP> host;
};

template <typename TP>
void vec_operand(xmca_handle* h, int side, const void* V, int64_t N, int64_t m, bool v_cplx, VecOperand<TP>& op) {
  if (!V) {
    const SolveResult& r = h->res;
    op.mode_major = true;
    op.ld = r.ldv[side];
    if constexpr (std::is_same<TP, float>::value) {
      XMCA_CHECK(r.vt_f32[side], XMCA_ERR_STATE, "transform: the resident vectors are not float32");
      op.r = r.Vt32[side].get();
    } else {
      XMCA_CHECK(!r.vt_f32[side], XMCA_ERR_STATE, "transform: the resident vectors are float32");
      op.r = r.Vt[side].r();
      op.i = r.Vt[side].i(r.cplx);
    }
    return;
  }
  op.mode_major = false;
  op.ld = m;
  upload_planes<TP>(h, static_cast<const double*>(V), (size_t)N * m, v_cplx, op.host);
  XMCA_HIP(hipStreamSynchronize(h->st));        // (the staging buffer goes back to the pool)
  op.host.stage.release();
  op.r = op.host.r;
  op.i = op.host.i;
}

// out (T_new x q) = (((X[:, keep] - mean) / std * weight) V[:, :m]) W   (see xmca_predict, xmca_predict_weighted).  TI: element type
// of the data (ingest arithmetic), TP: element type of the vectors (product).
template <typename TI, typename TP>
void predict_impl(xmca_handle* h, int side, const TI* X, bool x_dev, int64_t stride_t, int64_t stride_n, int64_t T, int64_t N_full,
                  const int64_t* keep_idx, int64_t N, const TI* mean,
                  const TI* stdv, const double* weight, const void* V, bool v_cplx, const double* W, int64_t m, int64_t q, bool w_cplx,
                  double* out, int* out_cplx) {
  VecOperand<TP> vo;
  vec_operand<TP>(h, side, V, N, m, v_cplx, vo);
  const bool vc = vo.i != nullptr, oc = vc || w_cplx;
  DevBuf<int64_t> idx;
  DevBuf<TI> mu, sd;
  DevBuf<double> wt;
  HostPlanes<double> w;
  if (keep_idx) XMCA_HIP(hipMemcpyAsync(idx.ensure((size_t)N), keep_idx, sizeof(int64_t) * N, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(mu.ensure((size_t)N), mean, sizeof(TI) * N, hipMemcpyHostToDevice, h->st));
  if (stdv) XMCA_HIP(hipMemcpyAsync(sd.ensure((size_t)N), stdv, sizeof(TI) * N, hipMemcpyHostToDevice, h->st));
  if (weight) XMCA_HIP(hipMemcpyAsync(wt.ensure((size_t)N), weight, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
  upload_planes<double>(h, W, (size_t)m * q, w_cplx, w, false);
  const double* Wr = w.r;
  const double* Wi = w.i;
  const int64_t rows = transform_rows(T, N_full * (int64_t)sizeof(TI) + N * (int64_t)sizeof(TP));
  DevBuf<TI> raw;
  DevBuf<TP> xs;
  DevBuf<double> yr, yi, o_r, o_i, packed;
  // new data on the device is not staged: rows that are contiguous are read in place with their pitch, any other view is made
  // contiguous block by block (ingest_strided)
  const bool in_place = x_dev && (stride_n == 1 || N_full == 1);
  if (!in_place) raw.ensure((size_t)rows * N_full);
  xs.ensure((size_t)rows * N);
  yr.ensure((size_t)rows * m);
  if (vc) yi.ensure((size_t)rows * m);
  o_r.ensure((size_t)rows * q);
  if (oc) { o_i.ensure((size_t)rows * q); packed.ensure((size_t)rows * q * 2); }
  for (int64_t t0 = 0; t0 < T; t0 += rows) {
    const int tb = (int)std::min<int64_t>(rows, T - t0);
    if (!x_dev) XMCA_HIP(hipMemcpyAsync(raw.get(), X + t0 * N_full, sizeof(TI) * tb * N_full, hipMemcpyHostToDevice, h->st));
    h->tm.begin("predict_ingest");
    if (x_dev && !in_place) ingest_strided<TI>(h->st, X + t0 * stride_t, tb, N_full, stride_t, stride_n, raw.get());
    hipLaunchKernelGGL((ingest_columns_kernel<TI, TP>), row_col_grid(tb, N), dim3(EW_BLOCK), 0, h->st,
                       in_place ? X + t0 * stride_t : raw.get(), in_place ? stride_t : N_full,
                       keep_idx ? idx.get() : nullptr, tb, N, mu.get(), stdv ? sd.get() : nullptr, weight ? wt.get() : nullptr,
                       xs.get());
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    h->tm.begin("predict_gemm");
    // Y = x V (tb x m): A = the ingested block, B(n, j) = V[:, j] at grid point n
    GemmOpts o;
    o.b_nfast = !vo.mode_major;
    gemm<TP, double>(h->st, h->gws, xs.get(), N, vo.r, vo.ld, yr.get(), m, tb, (int)m, (int)N, o);
    if (vc) gemm<TP, double>(h->st, h->gws, xs.get(), N, vo.i, vo.ld, yi.get(), m, tb, (int)m, (int)N, o);
    // out = Y W (tb x q, K = m):  Or = Yr Wr - Yi Wi,  Oi = Yr Wi + Yi Wr
    GemmOpts w;
    gemm<double, double>(h->st, h->gws, yr.get(), m, Wr, q, o_r.get(), q, tb, (int)q, (int)m, w);
    if (oc) {
      if (Wi) gemm<double, double>(h->st, h->gws, yr.get(), m, Wi, q, o_i.get(), q, tb, (int)q, (int)m, w);
      else XMCA_HIP(hipMemsetAsync(o_i.get(), 0, sizeof(double) * tb * q, h->st));
      if (vc) {
        GemmOpts acc;
        acc.beta = 1.0;
        gemm<double, double>(h->st, h->gws, yi.get(), m, Wr, q, o_i.get(), q, tb, (int)q, (int)m, acc);
        if (Wi) {
          acc.alpha = -1.0;
          gemm<double, double>(h->st, h->gws, yi.get(), m, Wi, q, o_r.get(), q, tb, (int)q, (int)m, acc);
        }
      }
    }
    h->tm.end();
    if (oc) {
      pack_download<double>(h, o_r.get(), o_i.get(), q, tb, (int)q, packed.get(), out + 2 * t0 * q);
    } else {          // (a real result needs no packing pass)
      XMCA_HIP(hipMemcpyAsync(out + t0 * q, o_r.get(), sizeof(double) * tb * q, hipMemcpyDeviceToHost, h->st));
    }
    XMCA_HIP(hipStreamSynchronize(h->st));      // (the pageable source / destination of the next block)
  }
  *out_cplx = oc ? 1 : 0;
}

// The finish of a reconstruction, shared by xmca_reconstruct* and xmca_extended_reconstruct: the compact tb x N product C of a block
// of rows goes to its final tb x N_full float64 layout (reconstruct_epilogue_kernel: / inv_weight, * std, + mean, NaN at the masked
// columns), on the device where the destination is there, else through a staging block.  `begin` uploads the per-column factors and
// sizes the row block; the caller fills C.get() (rows x N) and calls `finish` block by block.
struct ReconstructTail {
  DevBuf<int64_t> col_of;
  DevBuf<double> mu, sd, iw, C, full;
  int64_t N = 0, N_full = 0, rows = 0;
  bool out_dev = false;
  void begin(xmca_handle* h, int64_t T, const int64_t* keep_idx, int64_t N_, int64_t N_full_, const double* mean, const double* stdv,
             const double* inv_weight, bool out_dev_) {
    N = N_; N_full = N_full_; out_dev = out_dev_;
    upload_inverse_map(h, keep_idx, N, N_full, col_of);
    if (mean) XMCA_HIP(hipMemcpyAsync(mu.ensure((size_t)N), mean, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
    if (stdv) XMCA_HIP(hipMemcpyAsync(sd.ensure((size_t)N), stdv, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
    if (inv_weight) XMCA_HIP(hipMemcpyAsync(iw.ensure((size_t)N), inv_weight, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
    rows = transform_rows(T, (N + N_full) * (int64_t)sizeof(double));
  }
  void allocate() {
    C.ensure((size_t)rows * N);
    if (!out_dev) full.ensure((size_t)rows * N_full);
  }
  // rows [t0, t0 + tb) of the result from C; `timer`: the stage the epilogue is booked under
  void finish(xmca_handle* h, const char* timer, int64_t t0, int tb, double* out) {
    h->tm.begin(timer);
    hipLaunchKernelGGL(reconstruct_epilogue_kernel, row_col_grid(tb, N_full), dim3(EW_BLOCK), 0, h->st, C.get(), N,
                       col_of.get(), tb, N_full, iw.get(), sd.get(), mu.get(),      // (a buffer that was not filled is a null pointer)
                       out_dev ? out + t0 * N_full : full.get());                   // (a device destination is final)
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    if (!out_dev) {
      XMCA_HIP(hipMemcpyAsync(out + t0 * N_full, full.get(), sizeof(double) * tb * N_full, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipStreamSynchronize(h->st));
    }
  }
};

// out (T x N_full, float64) = Re(B V[:, :m]^H) / inv_weight * std + mean, NaN at the masked columns  (see xmca_reconstruct,
// xmca_reconstruct_weighted).  TP: element type of the vectors (product).
template <typename TP>
void reconstruct_impl(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, bool b_cplx, const void* V, bool v_cplx,
                      const int64_t* keep_idx, int64_t N, int64_t N_full, const double* mean, const double* stdv,
                      const double* inv_weight, double* out, bool out_dev) {
  VecOperand<TP> vo;
  if (m > 0) vec_operand<TP>(h, side, V, N, m, v_cplx, vo);
  const bool both_cplx = b_cplx && vo.i != nullptr;        // Re((Br + i Bi)(Vr - i Vi)^T) = Br Vr^T + Bi Vi^T
  ReconstructTail tail;
  tail.begin(h, T, keep_idx, N, N_full, mean, stdv, inv_weight, out_dev);
  HostPlanes<TP> bp;             // B in the product's element type
  if (m > 0) upload_planes<TP>(h, B, (size_t)T * m, b_cplx, bp);
  tail.allocate();
  const int64_t rows = tail.rows;
  for (int64_t t0 = 0; t0 < T; t0 += rows) {
    const int tb = (int)std::min<int64_t>(rows, T - t0);
    h->tm.begin("reconstruct_gemm");
    if (m == 0) {
      XMCA_HIP(hipMemsetAsync(tail.C.get(), 0, sizeof(double) * tb * N, h->st));
    } else {
      // C = B V^T (tb x N, K = m): A = the rows of B, B(j, n) = V[n, j]
      GemmOpts o;
      o.b_nfast = vo.mode_major;
      gemm<TP, double>(h->st, h->gws, bp.r + t0 * m, m, vo.r, vo.ld, tail.C.get(), N, tb, (int)N, (int)m, o);
      if (both_cplx) {
        o.beta = 1.0;
        gemm<TP, double>(h->st, h->gws, bp.i + t0 * m, m, vo.i, vo.ld, tail.C.get(), N, tb, (int)N, (int)m, o);
      }
    }
    h->tm.end();
    tail.finish(h, "reconstruct_epilogue", t0, tb, out);
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// checks shared by xmca_predict / xmca_reconstruct: the vectors (resident or host), the kept columns
void check_transform(xmca_handle* h, const char* what, int side, const void* V, int64_t m, const int64_t* keep_idx, int64_t N_keep,
                     int64_t N_full) {
  const std::string w(what);
  check_side(what, side);
  XMCA_CHECK(N_keep >= 1 && m >= 0 && m <= INT32_MAX, XMCA_ERR_INVALID, w + ": bad sizes");
  check_kept_columns(what, keep_idx, N_keep, N_full, INT32_MAX);
  if (!V && m > 0)
    XMCA_CHECK(h->solved && m <= h->res.n_vec && h->res.ldv[side] == N_keep, XMCA_ERR_INVALID,
               w + ": the resident vectors of the last solve do not have N_keep rows and m modes");
}

// C (N x m, device) = corr(Re field columns, Y columns): column moments, the tall GEMM X^T Y and pearson_finish_kernel; shared by
// xmca_correlate and xmca_correlation_maps.  `what`: the entry point's prefix of the message.
template <typename TI>
void correlate_device(xmca_handle* h, const char* what, int side, const double* Y, int64_t T, int64_t m, DevBuf<double>& C) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  XMCA_CHECK(f.T == T, XMCA_ERR_INVALID,
             std::string(what) + ": Y has " + std::to_string(T) + " rows, the field has " + std::to_string(f.T));
  const int64_t N = f.N;
  DevBuf<double> yh, sx, qx, sy, qy;
  DevBuf<TI> yt;
  const size_t ny = (size_t)T * m;
  XMCA_HIP(hipMemcpyAsync(yh.ensure(ny), Y, sizeof(double) * ny, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL((convert_kernel<double, TI>), ew_grid((int64_t)ny), dim3(EW_BLOCK), 0, h->st, yh.get(), yt.ensure(ny), (int64_t)ny);
  h->tm.begin("correlate");
  // (one chunk: cutting the rows would change the bits of the moments)
  column_pass(h->st, (int)T, N, 1, ColumnMoments<TI>{f.r(), N, sx.ensure((size_t)N), qx.ensure((size_t)N)});
  column_pass(h->st, (int)T, m, 1, ColumnMoments<double>{yh.get(), m, sy.ensure((size_t)m), qy.ensure((size_t)m)});
  XMCA_HIP(hipGetLastError());
  // C = X^T Y   (N x m): A(n, t) = X[t * N + n], B(t, j) = Y[t * m + j]
  GemmOpts o;
  o.a_kfast = false;
  gemm<TI, double>(h->st, h->gws, f.r(), N, yt.get(), m, C.ensure((size_t)N * m), m, (int)N, (int)m, (int)T, o);
  hipLaunchKernelGGL(pearson_finish_kernel, ew_grid(N * m), dim3(EW_BLOCK), 0, h->st, C.get(), N, (int)m, (int)T, sx.get(), qx.get(),
                     sy.get(), qy.get());
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  XMCA_HIP(hipStreamSynchronize(h->st));        // (Y is the caller's; the temporaries go back to the pool)
}

// r = corr(Re field columns, Y columns)  (see xmca_correlate)
template <typename TI>
void correlate_impl(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, double* r_out) {
  DevBuf<double> C;
  correlate_device<TI>(h, "correlate", side, Y, T, m, C);
  XMCA_HIP(hipMemcpyAsync(r_out, C.get(), sizeof(double) * (size_t)typed<TI>(h).f[side].N * m, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// p = 2 I_x(a, a) of `count` host values  (see xmca_pearson_pvalues)
void pearson_pvalues_impl(xmca_handle* h, const double* r, int64_t count, int64_t n_obs, double* p_out) {
  DevBuf<double> rd, pd;
  XMCA_HIP(hipMemcpyAsync(rd.ensure((size_t)count), r, sizeof(double) * count, hipMemcpyHostToDevice, h->st));
  h->tm.begin("pvalues");
  hipLaunchKernelGGL(pearson_pvalues_kernel, ew_grid(count), dim3(EW_BLOCK), 0, h->st, rd.get(), count, 0.5 * (double)n_obs - 1.0,
                     pvalue_log_norm(n_obs), pd.ensure((size_t)count));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(p_out, pd.get(), sizeof(double) * count, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// r (TR) and p (float64) of one field in their final N_full x m layout  (see xmca_correlation_maps)
template <typename TI, typename TR>
void correlation_maps_impl(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, const int64_t* keep_idx, int64_t N_full,
                           TR* r_out, double* p_out, bool out_dev) {
  DevBuf<double> C, pd;
  DevBuf<TR> rd;
  DevBuf<int64_t> row_of;
  correlate_device<TI>(h, "correlation_maps", side, Y, T, m, C);
  const int64_t N = typed<TI>(h).f[side].N;
  const int64_t* rows = upload_inverse_map(h, keep_idx, N, N_full, row_of);
  const size_t total = (size_t)N_full * m;
  h->tm.begin("correlation_maps");
  hipLaunchKernelGGL((correlation_maps_kernel<TR>), ew_grid((int64_t)total), dim3(EW_BLOCK), 0, h->st, C.get(), rows, N_full,
                     (int)m, 0.5 * (double)T - 1.0, pvalue_log_norm(T),
                     out_dev ? r_out : rd.ensure(total), out_dev ? p_out : pd.ensure(total));     // (device destinations are final)
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  if (!out_dev) {
    XMCA_HIP(hipMemcpyAsync(r_out, rd.get(), sizeof(TR) * total, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(p_out, pd.get(), sizeof(double) * total, hipMemcpyDeviceToHost, h->st));
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// x <- x - column means (T x N row-major), what the MCA constructor does to every surrogate / replicate (array.py:117):
// partial column sums over row chunks, means in a fixed order, one elementwise pass
template <typename TI>
void center_columns(xmca_handle* h, TI* x, int64_t T, int64_t N) {
  const int chunks = col_chunks(T);
  int* pn = h->center_nan.ensure((size_t)(chunks + 1) * N);      // (the finished values behind the partials, in plane `chunks`)
  double* ps = h->center_sum.ensure((size_t)(chunks + 1) * N);
  column_pass(h->st, (int)T, N, chunks, ColumnPartialSums<TI>{x, N, pn, ps});
  column_finish(h->st, N, ColumnFinishSums{pn, ps, chunks, (int)T, N, pn + (size_t)chunks * N, ps + (size_t)chunks * N});
  hipLaunchKernelGGL((subtract_column_means_kernel<TI>), ew_grid(T * N), dim3(EW_BLOCK), 0, h->st, x, (int)T, N, ps + (size_t)chunks * N);
  XMCA_HIP(hipGetLastError());
}

template <typename TI>
void center_field_impl(xmca_handle* h, int side, double* mean_out, double* std_out, int64_t* n_nan_out) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  XMCA_CHECK(!f.has_im && !f.ext_re, XMCA_ERR_STATE, "center_field: needs a real field owned by the library");
  const int64_t N = f.N;
  DevBuf<double> mean, sd, part_sum, part_sq;
  DevBuf<int> nans, part_nan;
  const int chunks = col_chunks(f.T), T = (int)f.T;
  part_nan.ensure((size_t)chunks * N);
  part_sum.ensure((size_t)chunks * N);
  part_sq.ensure((size_t)chunks * N);
  column_pass(h->st, T, N, chunks, ColumnPartialSums<TI>{f.re.get(), N, part_nan.get(), part_sum.get()});
  column_finish(h->st, N, ColumnFinishSums{part_nan.get(), part_sum.get(), chunks, T, N, nans.ensure((size_t)N), mean.ensure((size_t)N)});
  column_pass(h->st, T, N, chunks, CenterColumnsChunk<TI>{f.re.get(), N, mean.get(), nans.get(), part_sq.get()});
  column_finish(h->st, N, ColumnFinishStd{part_sq.get(), chunks, T, N, mean.get(), nans.get(), sd.ensure((size_t)N)});
  XMCA_HIP(hipGetLastError());
  std::vector<int> nh((size_t)N);
  XMCA_HIP(hipMemcpyAsync(mean_out, mean.get(), sizeof(double) * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(std_out, sd.get(), sizeof(double) * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(nh.data(), nans.get(), sizeof(int) * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  int64_t total = 0;
  for (int64_t c = 0; c < N; ++c) total += nh[(size_t)c];
  *n_nan_out = total;
}

// NaN-column handling of the constructor (array.py:191-197 `_set_no_nan_idx` / `_remove_nan_cols`) on the resident raw field:
// keep_out[c] = 1 for columns without a NaN; the field is replaced by its kept columns (T x n_keep).
template <typename TI>
void compact_field_impl(xmca_handle* h, int side, int* keep_out, int64_t* n_keep_out) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  XMCA_CHECK(!f.has_im && !f.ext_re, XMCA_ERR_STATE, "compact_field: needs a real field owned by the library");
  const int64_t N = f.N;
  DevBuf<int> nans, part_nan;
  const int chunks = col_chunks(f.T);
  part_nan.ensure((size_t)chunks * N);
  column_pass(h->st, (int)f.T, N, chunks, ColumnPartialSums<TI>{f.re.get(), N, part_nan.get(), nullptr});      // (no sum plane)
  column_finish(h->st, N, ColumnFinishSums{part_nan.get(), nullptr, chunks, (int)f.T, N, nans.ensure((size_t)N), nullptr});
  XMCA_HIP(hipGetLastError());
  std::vector<int> nh((size_t)N);
  XMCA_HIP(hipMemcpyAsync(nh.data(), nans.get(), sizeof(int) * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  std::vector<int64_t> idx;
  idx.reserve((size_t)N);
  for (int64_t c = 0; c < N; ++c) {
    keep_out[c] = nh[(size_t)c] == 0 ? 1 : 0;
    if (nh[(size_t)c] == 0) idx.push_back(c);
  }
  const int64_t nk = (int64_t)idx.size();
  *n_keep_out = nk;
  if (nk == N || nk == 0) return;     // nothing to drop / nothing left (the caller reports the latter its own way)
  DevBuf<int64_t> idx_dev;
  DevBuf<TI> out;
  XMCA_HIP(hipMemcpyAsync(idx_dev.ensure((size_t)nk), idx.data(), sizeof(int64_t) * nk, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL((gather_columns_kernel<TI>), ew_grid(f.T * nk), dim3(EW_BLOCK), 0, h->st, f.re.get(), N, out.ensure((size_t)(f.T * nk)), nk,
                     idx_dev.get(), (int)f.T);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipStreamSynchronize(h->st));   // idx goes out of scope
  f.re = std::move(out);
  f.N = nk;
}

// apply_weights / normalize of the constructor stage (array.py:317-365) on the resident centered field: one factor per column
template <typename TI>
void scale_field_impl(xmca_handle* h, int side, const void* w_host, int divide) {
  FieldData<TI>& f = typed<TI>(h).f[side];
  XMCA_CHECK(!f.has_im && !f.ext_re, XMCA_ERR_STATE, "scale_field: needs a real field owned by the library");
  DevBuf<TI> w;
  XMCA_HIP(hipMemcpyAsync(w.ensure((size_t)f.N), w_host, sizeof(TI) * (size_t)f.N, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL((scale_columns_kernel<TI>), ew_grid(f.T * f.N), dim3(EW_BLOCK), 0, h->st, f.re.get(), (int)f.T, f.N, w.get(), divide);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipStreamSynchronize(h->st));
}

void fill_rot_outputs(const RotateResult& rr, bool cplx, double* R_out, double* Phi_out, double* nl, double* nr, int* iters) {
  const int p = rr.p;
  if (iters) *iters = rr.iters;
  for (int e = 0; e < p * p; ++e) {
    if (cplx) {
      if (R_out) { R_out[2 * e] = rr.R[e].real(); R_out[2 * e + 1] = rr.R[e].imag(); }
      if (Phi_out) { Phi_out[2 * e] = rr.Phi[e].real(); Phi_out[2 * e + 1] = rr.Phi[e].imag(); }
    } else {
      if (R_out) R_out[e] = rr.R[e].real();
      if (Phi_out) Phi_out[e] = rr.Phi[e].real();
    }
  }
  for (int k = 0; k < p; ++k) {
    if (nl && !rr.norm_left.empty()) nl[k] = rr.norm_left[k];
    if (nr && !rr.norm_right.empty()) nr[k] = rr.norm_right[k];
  }
}

void check_rot(const RotateResult& rr) {
  XMCA_CHECK(!rr.nan, XMCA_ERR_NUMERIC, "varimax: NaN encountered (zero or NaN rows in the loadings?)");
  XMCA_CHECK(rr.converged, XMCA_ERR_NOT_CONVERGED,
             "Rotation process did not converge. Try decreasing the tolerance. Invalid NaN entries also might be a problem.");
}

// Promax of the first p modes of `res` where its vectors are (array.py:815-833): the loadings V sqrt(sigma) of both fields
// stacked (array.py:818-822; Nl left rows, Nr right rows, 0 for a one-field result) are built in `d`, then rotated.
// `lead_left` (xmca_rotate_solved beside a deferred tail): where the leading modes of the real left field are until the join.
void rotate_resident(xmca_handle* h, Rotator& rot, RotationDevice& d, DevBuf<double>& sigma_dev, const SolveResult& res, int64_t Nl,
                     int64_t Nr, int p, int power, double tol, int max_iter, RotateResult& rr, const double* lead_left = nullptr) {
  const bool cplx = res.cplx;
  rot.alloc(d, Nl + Nr, Nl, p, cplx);
  XMCA_HIP(hipMemcpyAsync(sigma_dev.ensure((size_t)p), res.sigma.data(), sizeof(double) * p, hipMemcpyHostToDevice, h->st));
  const CPlanes& Vl = res.Vt[0];
  const CPlanes& Vr = res.Vt[Nr > 0 ? 1 : 0];
  if (res.vt_f32[0]) {
    // float32 model (one real field): the reference multiplies the float32 vectors by the float32 square roots of the float32
    // singular values - a float32 product - and rotates that; the same roundings here, then float64 like the host path
    XMCA_CHECK(!cplx && Nr == 0, XMCA_ERR_STATE, "rotate: float32-resident vectors are real and one-sided");
    hipLaunchKernelGGL(rot_build_loadings_f32_kernel, ew_grid(Nl), dim3(EW_BLOCK), 0, h->st, res.Vt32[0].get(), Nl, Nl, sigma_dev.get(), p,
                       d.A.r(), d.h.get());
  } else if (cplx) {
    hipLaunchKernelGGL((rot_build_loadings_kernel<true>), ew_grid(Nl + Nr), dim3(EW_BLOCK), 0, h->st, Vl.r(), Vl.i(true), Nl, Nl,
                       Vr.r(), Vr.i(true), Nr > 0 ? Nr : Nl, Nr, sigma_dev.get(), p, d.A.r(), d.A.i(true), d.h.get());
  } else {
    hipLaunchKernelGGL((rot_build_loadings_kernel<false>), ew_grid(Nl + Nr), dim3(EW_BLOCK), 0, h->st, lead_left ? lead_left : Vl.r(),
                       (const double*)nullptr, Nl, Nl, Vr.r(), (const double*)nullptr, Nr > 0 ? Nr : Nl, Nr, sigma_dev.get(), p, d.A.r(),
                       (double*)nullptr, d.h.get());
  }
  rot.run(d, power, tol, max_iter, rr, nullptr, false);
}

// What every replicate of a rule_n / bootstrap call has in common: the shape of the fields, the complexification (op == nullptr:
// real replicates) and the rotation (rotated != 0: n_rot = p, power, tol)
struct ReplicateSpec {
  int64_t T = 0, Nx = 0, Ny = 0;
  int n_fields = 1;
  const ComplexOp* op = nullptr;
  int rotated = 0, p = 0, power = 1;
  double tol = 0.0;
  int n_vec = 0;     // unrotated replicates: back-project the vectors of this many leading modes (xmca_bootstrap_patterns)
  int64_t eig_n() const { return std::min(T, n_fields == 2 ? std::min(Nx, Ny) : Nx); }     // order of the eigenproblems = rank
};

// One surrogate / bootstrap replicate from centered real fields resident in `f` (re planes): complexify, solve, rotate,
// variance spectrum (the body of the loops array.py:1753-1765 and :1935-1947).
template <typename TI>
struct ReplicateRunner {
  xmca_handle* h;
  int64_t T, Ns[2];
  int n_fields, rotated, p, power, n_vec;
  double tol;
  bool cplx, analytic;
  DevBuf<TI> htb;
  // extend='theta' (ComplexOp::THETA): the lane's own copy of B and one fit buffer per field, 2 (THETA_HEAD + m) x N, reused by
  // every replicate of the lane.  The season kernel accumulates its phase sums in the fit buffer: no two lanes may share one.
  int period = 0, kb = 0;
  DevBuf<double> bdev, fit[2];
  Solver<TI> solver;
  Rotator rot;
  SolveResult res;
  RotationDevice rd;
  DevBuf<double> sigma_dev;

  ReplicateRunner(xmca_handle* h_, const ReplicateSpec& s)
      : h(h_), T(s.T), Ns{s.Nx, s.Ny}, n_fields(s.n_fields), rotated(s.rotated), p(s.p), power(s.power), n_vec(s.n_vec),
        tol(s.tol), cplx(s.op != nullptr),
        solver(h_->st, h_->gws, h_->ews, h_->tm), rot(h_->st, h_->tm, h_->gws, h_->ews) {
    const ComplexOp* op = s.op;
    // vectors of n_vec modes wanted (xmca_bootstrap_patterns): a one-field replicate forms only those eigenvectors, as
    // xmca_solve does for solve(n_modes=k); the values-only and rotated replicates keep their routes - their bits are pinned
    solver.partial_vectors = n_vec > 0;
    analytic = cplx && Solver<TI>::analytic_route(op->kind == ComplexOp::CIRCULANT, T, s.Nx, s.Ny, n_fields, false);
    if (cplx) XMCA_CHECK(op->T == T, XMCA_ERR_INVALID, "replicates: the operator was made for another number of time steps");
    if (cplx && op->kind == ComplexOp::THETA) {
      XMCA_CHECK((std::is_same<TI, double>::value), XMCA_ERR_INVALID, "replicates: the Theta extension needs float64 fields");
      period = op->period;
      kb = (int)(2 * theta_fit_rows(period));
      XMCA_CHECK(period >= 1 && T >= 2 * (int64_t)period && (int64_t)op->B.size() == T * kb, XMCA_ERR_STATE,
                 "replicates: inconsistent parts of the Theta extension");
      // (the copy has landed when build_operator below has synchronised the stream)
      XMCA_HIP(hipMemcpyAsync(bdev.ensure(op->B.size()), op->B.data(), sizeof(double) * op->B.size(), hipMemcpyHostToDevice, h->st));
      for (int k = 0; k < n_fields; ++k) fit[k].ensure((size_t)kb * Ns[k]);
    }
    if (cplx && !analytic) build_operator<TI>(h, *op, htb);
  }
  int64_t rank() const { return std::min(T, n_fields == 2 ? std::min(Ns[0], Ns[1]) : Ns[0]); }

  // f[s].re holds the centered field; returns 1 (kept) or 0 (Varimax failed: the replicate is dropped, array.py:1762-1763)
  int run(FieldData<TI>* f, double* out, int64_t n_out) {
    if constexpr (std::is_same<TI, double>::value) {
      if (kb > 0) {     // the Theta fits C of the centred replicate, as complexify_impl fits the resident field
        h->tm.begin("theta_fit");
        for (int s = 0; s < n_fields; ++s) theta_fit(h->st, f[s].r(), T, Ns[s], period, fit[s].get());
        h->tm.end();
      }
    }
    for (int s = 0; s < n_fields; ++s) {
      f[s].has_im = false;
      if (cplx && !analytic) apply_operator<TI>(h, htb.get(), kb > 0 ? bdev.get() : nullptr, fit[s].get(), kb, f[s]);
    }
    if (analytic) solver.solve_analytic(f, n_fields, rotated ? p : n_vec, res);
    else solver.solve(f, n_fields, cplx, rotated ? p : n_vec, res);
    if (!rotated) {
      for (int64_t i = 0; i < n_out; ++i) out[i] = res.sigma[i];
      return 1;
    }
    RotateResult rr;
    rotate_resident(h, rot, rd, sigma_dev, res, Ns[0], n_fields == 2 ? Ns[1] : 0, p, power, tol, 1000, rr);
    if (rr.nan || !rr.converged) {       // array.py:1762-1763: the run is silently dropped
      for (int64_t i = 0; i < n_out; ++i) out[i] = 0.0;
      return 0;
    }
    std::vector<double> var(p);
    for (int k = 0; k < p; ++k) var[k] = n_fields == 2 ? rr.norm_left[k] * rr.norm_right[k] : rr.norm_left[k] * rr.norm_left[k];
    std::sort(var.begin(), var.end(), [](double a, double b) { return a > b; });
    for (int k = 0; k < p; ++k) out[k] = var[k];
    return 1;
  }
};

// The replicates run = first, first + stride, ... < n_runs of one lane of a rule_n / bootstrap call (`what`).  fill(side, x, run)
// queues the raw real field of `side` (T x N, row-major) into x on the lane's stream; the field is centered like the MCA
// constructor does (array.py:117) and handed to the runner.  `stage` names the stage timer of that preparation.  sync_each_run:
// the stream is synchronised after every replicate (a fill that uploads from a buffer it reuses for the next replicate), else
// once when the lane has queued its last one.  after(run, result), when given, queues what the caller makes of the replicate's
// vectors (spec.n_vec modes) behind its solve, before that synchronisation.
template <typename TI, typename Fill>
void replicate_lane(xmca_handle* h, const char* what, const char* stage, const ReplicateSpec& spec, int64_t first, int64_t stride,
                    int64_t n_runs, bool sync_each_run, double* spectra, int* kept, int64_t n_out, Fill&& fill,
                    const std::function<void(int64_t, const SolveResult&)>& after = nullptr) {
  FieldData<TI> f[2];
  const int64_t T = spec.T, Ns[2] = {spec.Nx, spec.Ny};
  ReplicateRunner<TI> runner(h, spec);
  XMCA_CHECK(n_out == (spec.rotated ? (int64_t)spec.p : spec.n_vec > 0 ? (int64_t)spec.n_vec : runner.rank()), XMCA_ERR_INVALID,
             std::string(what) + ": n_out must be rank (unrotated), p (rotated) or the modes whose vectors are wanted");
  for (int64_t run = first; run < n_runs; run += stride) {
    h->tm.begin(stage);
    for (int s = 0; s < spec.n_fields; ++s) {
      f[s].T = T; f[s].N = Ns[s]; f[s].has_im = false; f[s].ext_re = nullptr;
      TI* x = f[s].re.ensure((size_t)(T * Ns[s]));
      fill(s, x, run);
      XMCA_HIP(hipGetLastError());
      center_columns<TI>(h, x, T, Ns[s]);
    }
    h->tm.end();
    kept[run] = runner.run(f, spectra + run * n_out, n_out);
    if (after) after(run, runner.res);
    if (sync_each_run) XMCA_HIP(hipStreamSynchronize(h->st));
  }
  if (!sync_each_run) XMCA_HIP(hipStreamSynchronize(h->st));
}

// Surrogates are independent: `lanes` of them are in flight at a time, each on its own stream with its own workspaces
// and host thread (the solver synchronises its stream now and then, so a lane needs a thread of its own).  A round of
// the eigensolver leaves the chip partly idle - its tile-solve chain and the tail of its updates - and a
// second surrogate's kernels fill that: measured at C4 as two PROCESSES sharing the GPU +34 % surrogates/s
// (profiles/r02_bench_shared_gpu_2ranks.json), now inside one process.  Lane j takes the runs j, j + lanes, ...; the
// generator is keyed by (seed, run, side), so the spectra do not depend on the number of lanes.  XMCA_RULE_N_LANES
// (default: 2 for eigenproblems of 2000 and more, 4 below; 1 = the plain loop).
//
// number of replicates kept in flight
static int lanes_for(int64_t eig_n, int64_t n_runs) {
  // measured on MI355X (scripts/rule_n_bench.py, surrogates/s with 1 / 2 / 3 / 4 lanes): C4 8.0 / 10.6 / 10.4 / 10.4,
  // C2-shaped EOF 25.8 / 32.9 / 33.1 / 32.3, C1-shaped (eigenproblems of 675) 109 / 191 / 265 / 337
  static const int lanes_env = [] { const char* e = std::getenv("XMCA_RULE_N_LANES"); return e ? std::max(1, std::min(8, std::atoi(e))) : 0; }();
  // (round 4, contiguous row ownership in the persistent reduction - its workgroups leave from early on: C4 with 2 / 3 / 4 / 5
  //  lanes 48.2 / 45.9 / 45.9 / 47.0 ms per surrogate; C2-shaped EOF and the rotated cases do not care)
  // (round 5, left-looking Cholesky of ~80 small launches and the faster reduction: C4 with 1 / 2 / 3 / 4 lanes 19.0 / 22.9 / 20.1 /
  //  18.7 surrogates/s, C4 rotated 8.8 / 10.9 / 9.3 / 8.0, C2-shaped EOF 42.0 / 44.2 / 44.1 / 43.9 (scripts/lanes_sweep.py): a third
  //  lane now costs more in interleaved small launches than it fills)
  const int lanes_wanted = lanes_env ? lanes_env : (eig_n >= 2000 ? 2 : 4);
  return (int)std::min<int64_t>(lanes_wanted, std::max<int64_t>(n_runs, 1));
}

// body(lane handle, j) on `lanes` host threads (lane 0 = the caller's handle on the calling thread); the first error is
// rethrown after every lane has been joined; stage times and round counters of the lanes are added to the caller's.
template <typename F>
void run_lanes(xmca_handle* h, int lanes, F&& lane_body) {
  while ((int)h->lanes.size() < lanes - 1) {
    xmca_handle* lane = nullptr;
    XMCA_CHECK(xmca_create(h->device, &lane) == XMCA_OK, XMCA_ERR_HIP, "cannot create a lane (stream)");
    h->lanes.push_back(lane);
  }
  std::vector<std::exception_ptr> errs((size_t)lanes);
  std::vector<std::thread> threads;
  auto body = [&](int j) {
    xmca_handle* lh = j == 0 ? h : h->lanes[(size_t)j - 1];
    try {
      ::xmca::PoolScope scope(&lh->pool);
      XMCA_HIP(hipSetDevice(h->device));
      lh->tm.enabled = h->tm.enabled;
      struct LaneFlag {
        bool prev;
        explicit LaneFlag(bool on) : prev(::xmca::in_surrogate_lanes()) { ::xmca::in_surrogate_lanes() = on; }
        ~LaneFlag() { ::xmca::in_surrogate_lanes() = prev; }
      } flag(lanes > 1);
      lane_body(lh, j);
      XMCA_HIP(hipStreamSynchronize(lh->st));
    } catch (...) {
      errs[(size_t)j] = std::current_exception();
      (void)hipStreamSynchronize(lh->st);
    }
  };
  for (int j = 1; j < lanes; ++j) threads.emplace_back(body, j);
  body(0);
  for (auto& t : threads) t.join();
  for (xmca_handle* lane : h->lanes) {
    lane->tm.collect();
    for (const auto& name : lane->tm.order) {
      if (!h->tm.ms.count(name)) h->tm.order.push_back(name);
      h->tm.ms[name] += lane->tm.ms[name];
    }
    lane->tm.ms.clear();
    lane->tm.order.clear();
    h->ews.round_ms += lane->ews.round_ms; h->ews.round_launches += lane->ews.round_launches;
    lane->ews.round_ms = 0.0;
    lane->ews.round_launches = 0;
    h->ews.trd.reduce_ms += lane->ews.trd.reduce_ms; h->ews.trd.reduce_calls += lane->ews.trd.reduce_calls;
    h->ews.trd.resident_calls += lane->ews.trd.resident_calls;
    lane->ews.trd.reduce_ms = 0.0; lane->ews.trd.reduce_calls = 0; lane->ews.trd.resident_calls = 0;
  }
  // memory parked in the lane pools is of no use to anybody until the next rule_n / bootstrap call: give large amounts back
  // (every lane stream has been synchronised above)
  size_t parked = 0;
  for (xmca_handle* lane : h->lanes) { std::lock_guard<std::mutex> g(lane->pool.mu); parked += lane->pool.held; }
  if (parked > ((size_t)4 << 30))
    for (xmca_handle* lane : h->lanes) lane->pool.trim();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
}

// lane_body(lane handle, first, stride) runs the replicates first, first + stride, ... of a rule_n / bootstrap call: on the
// caller's handle alone (the plain loop), or on as many concurrent lanes as lanes_for grants
template <typename F>
void run_replicates(xmca_handle* h, const ReplicateSpec& spec, int64_t n_runs, F&& lane_body) {
  const int lanes = lanes_for(spec.eig_n(), n_runs);
  if (lanes <= 1) {
    lane_body(h, (int64_t)0, (int64_t)1);
    return;
  }
  run_lanes(h, lanes, [&](xmca_handle* lh, int j) { lane_body(lh, (int64_t)j, (int64_t)lanes); });
}

// Queues the AR(1) recurrence (kernels.h) over the T x N plane of normals in x, in place.  phi: N values on the
// device; carry: scratch of the calling lane, (segments - 1) x N.
template <typename TI>
void ar1_filter(hipStream_t st, TI* x, int64_t T, int64_t N, const double* phi, DevBuf<double>& carry) {
  const Ar1Segments seg = ar1_segments(T, N);
  const unsigned gx = (unsigned)ceil_div(N, (int64_t)AR1_BLOCK);
  double* cr = nullptr;
  if (seg.count > 1) {
    cr = carry.ensure((size_t)((seg.count - 1) * N));
    hipLaunchKernelGGL((ar1_carry_kernel<TI>), dim3(gx, (unsigned)(seg.count - 1)), dim3(AR1_BLOCK), 0, st, (const TI*)x, T, N, seg.length,
                       phi, cr);
  }
  hipLaunchKernelGGL((ar1_filter_kernel<TI>), dim3(gx, (unsigned)seg.count), dim3(AR1_BLOCK), 0, st, x, T, N, seg.length, phi,
                     (const double*)cr);
}

// every phi finite and inside (-1, 1): checked on the host before anything is launched
void check_phi(const char* what, const double* phi, int64_t N) {
  XMCA_CHECK(phi != nullptr, XMCA_ERR_INVALID, std::string(what) + ": phi is missing");
  for (int64_t c = 0; c < N; ++c)
    XMCA_CHECK(std::fabs(phi[c]) < 1.0, XMCA_ERR_INVALID, std::string(what) + ": every phi must be finite with |phi| < 1");   // (false for NaN)
}

// runs [run_begin, run_end) of xmca_rule_n: the fields of run r are N(0,1) surrogates keyed by (seed, r, side); with phi (device
// pointers of Nx / Ny values that every lane only reads) they are filtered into AR(1) columns, xmca_rule_n_ar1
template <typename TI>
void rule_n_impl(xmca_handle* h, const ReplicateSpec& spec, int64_t run_begin, int64_t run_end, uint64_t seed, double* spectra, int* kept,
                 int64_t n_out, const double* const* phi = nullptr) {
  const int64_t Ns[2] = {spec.Nx, spec.Ny};
  run_replicates(h, spec, run_end - run_begin, [&](xmca_handle* lh, int64_t first, int64_t stride) {
    DevBuf<double> carry;      // the lane's own: reused by its replicates in stream order
    replicate_lane<TI>(lh, "rule_n", "surrogate", spec, first, stride, run_end - run_begin, false, spectra, kept, n_out,
                       [&](int s, TI* x, int64_t run) {
                         const int64_t n = spec.T * Ns[s];
                         hipLaunchKernelGGL((philox_normal_kernel<TI>), ew_grid((n + 1) / 2), dim3(EW_BLOCK), 0, lh->st, x, n, seed,
                                            (uint32_t)(run_begin + run), (uint32_t)s);
                         if (phi) ar1_filter<TI>(lh->st, x, spec.T, Ns[s], phi[s], carry);
                       });
  });
}

// xmca_lag1_autocorrelation: phi of the columns of the resident real plane of `side`, chunked like the column passes of the
// constructor and finished in a fixed order
template <typename TI>
void lag1_impl(xmca_handle* h, int side, double* phi_out) {
  const FieldData<TI>& f = typed<TI>(h).f[side];
  const int64_t T = f.T, N = f.N;
  XMCA_CHECK(T >= 2 && N >= 1, XMCA_ERR_STATE, "lag1_autocorrelation: the field needs at least 2 time steps");
  const int chunks = col_chunks(T);
  DevBuf<double> part, ends, phi;
  column_pass(h->st, (int)T, N, chunks, Lag1Partial<TI>{f.r(), (int)T, N, part.ensure((size_t)3 * chunks * N), ends.ensure((size_t)2 * N)});
  column_finish(h->st, N, Lag1Finish{part.get(), ends.get(), chunks, (int)T, N, phi.ensure((size_t)N)});
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(phi_out, phi.get(), sizeof(double) * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// xmca_surrogate_ar1: the filtered, uncentred field of one run in the run dtype, widened to float64 on the host
template <typename TI>
void surrogate_ar1_impl(xmca_handle* h, int64_t T, int64_t N, const double* phi, uint64_t seed, uint32_t run, uint32_t side, double* out) {
  const int64_t n = T * N;
  DevBuf<TI> x;
  DevBuf<double> phi_dev, carry, wide;
  XMCA_HIP(hipMemcpyAsync(phi_dev.ensure((size_t)N), phi, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL((philox_normal_kernel<TI>), ew_grid((n + 1) / 2), dim3(EW_BLOCK), 0, h->st, x.ensure((size_t)n), n, seed, run, side);
  ar1_filter<TI>(h->st, x.get(), T, N, phi_dev.get(), carry);
  hipLaunchKernelGGL((convert_kernel<TI, double>), ew_grid(n), dim3(EW_BLOCK), 0, h->st, (const TI*)x.get(), wide.ensure((size_t)n), n);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(out, wide.get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// ---- bootstrap statistics of the vectors (boot_patterns.h) ------------------------------------------------
// What one xmca_bootstrap_patterns / xmca_pattern_stats call keeps on the device: the model's vectors (uploaded once; the lanes
// only read them), one set of float64 accumulators per lane and side, and the congruence of every run.  Allocated from the
// caller's pool on the caller's stream and synchronised (begin) before a lane touches it.
struct PatternStats {
  int k = 0, n_sides = 1, lanes = 1;
  bool cplx = false;
  int64_t N[2] = {0, 0}, n_runs = 0;
  int tile_off[2] = {0, 0}, total_tiles = 0;
  DevBuf<double> v0_re[2], v0_im[2], acc[2], g;
  int ncomp() const { return cplx ? 3 : 2; }
  size_t kN(int s) const { return (size_t)k * (size_t)N[s]; }
  double* lane_acc(int s, int lane, int comp) const { return acc[s].get() + ((size_t)lane * ncomp() + comp) * kN(s); }

  void begin(xmca_handle* h, const double* const v0_re_host[2], const double* const v0_im_host[2]) {
    int64_t tiles = 0;
    for (int s = 0; s < n_sides; ++s) {
      tile_off[s] = (int)tiles;
      tiles += pattern_tiles(N[s]);
      XMCA_HIP(hipMemcpyAsync(v0_re[s].ensure(kN(s)), v0_re_host[s], sizeof(double) * kN(s), hipMemcpyHostToDevice, h->st));
      if (cplx) XMCA_HIP(hipMemcpyAsync(v0_im[s].ensure(kN(s)), v0_im_host[s], sizeof(double) * kN(s), hipMemcpyHostToDevice, h->st));
      const size_t n_acc = (size_t)lanes * ncomp() * kN(s);
      XMCA_HIP(hipMemsetAsync(acc[s].ensure(n_acc), 0, sizeof(double) * n_acc, h->st));
    }
    XMCA_CHECK(tiles <= INT32_MAX / 4, XMCA_ERR_UNSUPPORTED, "pattern statistics: too many columns");
    total_tiles = (int)tiles;
    g.ensure((size_t)(n_runs * k));
    XMCA_HIP(hipStreamSynchronize(h->st));
  }

  // the three per-replicate kernels on `st`: vectors of run `run` (planes of TV, k rows of stride ldv; im nullptr when real)
  // into the accumulators of `lane`; part (2 k total_tiles) and u (2 k) are scratch of the calling lane
  template <typename TV>
  void queue(hipStream_t st, int lane, int64_t run, const TV* const v_re[2], const TV* const v_im[2], const int64_t ldv[2], double* part,
             double* u) const {
    for (int s = 0; s < n_sides; ++s)
      hipLaunchKernelGGL((pattern_dot_partial_kernel<TV>), dim3((unsigned)pattern_tiles(N[s]), (unsigned)k), dim3(PATTERN_BLOCK), 0, st,
                         (const double*)v0_re[s].get(), (const double*)(cplx ? v0_im[s].get() : nullptr), N[s], v_re[s],
                         cplx ? v_im[s] : (const TV*)nullptr, ldv[s], N[s], tile_off[s], total_tiles, part);
    hipLaunchKernelGGL(pattern_phase_kernel, dim3((unsigned)ceil_div((int64_t)k, (int64_t)64)), dim3(64), 0, st, (const double*)part, total_tiles,
                       k, n_sides, u, g.get() + run * k);
    for (int s = 0; s < n_sides; ++s)
      hipLaunchKernelGGL((pattern_accumulate_kernel<TV>), dim3((unsigned)ceil_div(N[s], (int64_t)PATTERN_BLOCK), (unsigned)k),
                         dim3(PATTERN_BLOCK), 0, st, (const double*)v0_re[s].get(), (const double*)(cplx ? v0_im[s].get() : nullptr), N[s],
                         v_re[s], cplx ? v_im[s] : (const TV*)nullptr, ldv[s], N[s], (const double*)u, lane_acc(s, lane, 0),
                         cplx ? lane_acc(s, lane, 1) : (double*)nullptr, lane_acc(s, lane, ncomp() - 1));
    XMCA_HIP(hipGetLastError());
  }

  // the vectors of a replicate's result, in whichever planes its solve left them
  void queue_result(hipStream_t st, int lane, int64_t run, const SolveResult& r, double* part, double* u) const {
    XMCA_CHECK(r.n_vec >= k && r.cplx == cplx, XMCA_ERR_STATE, "bootstrap_patterns: the replicate has not the vectors asked for");
    for (int s = 0; s < n_sides; ++s)
      XMCA_CHECK(r.ldv[s] == N[s] && r.vt_f32[s] == r.vt_f32[0], XMCA_ERR_STATE, "bootstrap_patterns: unexpected layout of the replicate's vectors");
    if (r.vt_f32[0]) {
      XMCA_CHECK(!cplx, XMCA_ERR_STATE, "bootstrap_patterns: float32-resident vectors are real");
      const float* re[2] = {r.Vt32[0].get(), r.Vt32[1].get()};
      const float* im[2] = {nullptr, nullptr};
      queue<float>(st, lane, run, re, im, r.ldv, part, u);
    } else {
      const double* re[2] = {r.Vt[0].r(), r.Vt[1].r()};
      const double* im[2] = {r.Vt[0].i(cplx), r.Vt[1].i(cplx)};
      queue<double>(st, lane, run, re, im, r.ldv, part, u);
    }
  }

  // after every lane's stream has been synchronised: merge in lane order, download (mean interleaved when complex)
  void finish(xmca_handle* h, double* const mean_out[2], double* const std_out[2], double* congruence_out) {
    DevBuf<double> mean[2], sd[2];
    for (int s = 0; s < n_sides; ++s) {
      const size_t n = kN(s), nm = n * (cplx ? 2 : 1);
      hipLaunchKernelGGL(pattern_merge_kernel, ew_grid((int64_t)n), dim3(EW_BLOCK), 0, h->st, (const double*)acc[s].get(), lanes, cplx ? 1 : 0,
                         (int64_t)n, (const double*)v0_re[s].get(), (const double*)(cplx ? v0_im[s].get() : nullptr), (double)n_runs,
                         mean[s].ensure(nm), sd[s].ensure(n));
      XMCA_HIP(hipGetLastError());
      XMCA_HIP(hipMemcpyAsync(mean_out[s], mean[s].get(), sizeof(double) * nm, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(std_out[s], sd[s].get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
    }
    XMCA_HIP(hipMemcpyAsync(congruence_out, g.get(), sizeof(double) * (size_t)(n_runs * k), hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
  }
};

// ---- extended (lag-embedded) EOFs (csrc/lag_gram.h, csrc/lag_reconstruct.h) -----------------------------
// Back-projection of leading vectors on the lagged views of a plane: Z (q x Tp, float64) is narrowed to the plane's element type
// into the caller's `z`, then one thin GEMM per lag j < M of Z against the rows [j tau, j tau + Tp) of X (T x N, row stride N)
// fills the rows [j q, (j + 1) q) of P, row c times row_scale[c] where that is given.  xmca_fill_gaps is the case M = 1.
template <typename TI>
void lag_back_project(xmca_handle* h, Narrow<TI>& z, const double* Z, int q, int Tp, int M, int tau, const TI* X, int64_t N,
                      const double* row_scale, double* P) {
  z.from(h->st, Z, nullptr, (int64_t)q * Tp);
  for (int j = 0; j < M; ++j) {
    GemmOpts o;
    o.a_kfast = true; o.b_nfast = true;
    o.row_scale = row_scale;
    gemm<TI, double>(h->st, h->gws, z.r, Tp, X + (int64_t)j * tau * N, N, P + (int64_t)j * q * N, N, q, (int)N, Tp, o);
  }
}

// The front shared by xmca_extended_eofs and xmca_extended_reconstruct: Gram product of the resident field of side 0, lag sum and
// double centring, the k leading eigenvectors Z (k x T', row c the vector of mode c) and all eigenvalues `lam` of the T' x T' matrix.
// The buffers live as long as the struct: the caller keeps it for the whole call.
struct EeofFront {
  CPlanes G;
  DevBuf<double> K, part, mean, Z, lam_dev;
  std::vector<double> lam;
};

template <typename TI>
void eeof_leading_vectors(xmca_handle* h, const char* what, int M, int tau, int k, EeofFront& w) {
  const FieldData<TI>& f = typed<TI>(h).f[0];
  const int T = (int)f.T, np = T - (M - 1) * tau;
  Solver<TI> s(h->st, h->gws, h->ews, h->tm);
  s.gram(f, false, w.G);
  h->tm.begin("lag_gram");
  lag_gram(h->st, w.G.r(), T, T, M, tau, true, w.K.ensure((size_t)np * np), w.part, w.mean);
  h->tm.end();
  EvdInfo info;
  h->tm.begin("eeof_eigh");
  hermitian_evd(h->st, h->ews, w.K.get(), nullptr, np, np, w.lam, w.lam_dev.ensure((size_t)np), w.Z.ensure((size_t)k * np), nullptr, np, &info,
                false, k < np ? k : -1);
  XMCA_HIP(hipStreamSynchronize(h->st));
  h->tm.end();
  XMCA_CHECK(std::isfinite(w.lam[0]) && w.lam[0] > 0.0, XMCA_ERR_NUMERIC, std::string(what) + ": the field has no variance (or holds NaN)");
}

// The patterns of the k leading modes of a front, shared by xmca_extended_eofs and the Monte-Carlo SSA entries: P (M planes of
// k x N, row c of plane j the lag-j pattern of mode c) and scale (k values: P times scale has unit norm over lags x points and
// the sign of the sign rule).  Stage timer "eeof_project".  The buffers, and the host values on their way up, live as long as the
// struct: the caller keeps it until it has synchronised the stream.
template <typename TI>
struct EeofPatterns {
  std::vector<double> inv;
  DevBuf<double> inv_dev, P, scale;
  Narrow<TI> z;
};

template <typename TI>
void eeof_patterns(xmca_handle* h, const EeofFront& front, int M, int tau, int k, EeofPatterns<TI>& w) {
  const FieldData<TI>& f = typed<TI>(h).f[0];
  const int np = (int)f.T - (M - 1) * tau;
  const int64_t N = f.N, plane = (int64_t)k * N;
  const std::vector<double>& lam = front.lam;
  // 1 / sigma_c rides in the epilogue for the modes clear of the Gram matrix's rounding noise (the cuts of the one-field solve);
  // the others are divided by their measured norm afterwards (eeof_sign_norm_kernel)
  const double cut = (std::is_same<TI, float>::value ? 1e-4 : 1e-6) * lam[0];
  std::vector<double>& inv = w.inv;
  inv.assign((size_t)k, 1.0);
  int known = 0;
  while (known < k && lam[(size_t)known] > cut) { inv[(size_t)known] = 1.0 / std::sqrt(lam[(size_t)known]); ++known; }
  XMCA_HIP(hipMemcpyAsync(w.inv_dev.ensure((size_t)k), inv.data(), sizeof(double) * k, hipMemcpyHostToDevice, h->st));
  w.P.ensure((size_t)M * plane);
  h->tm.begin("eeof_project");
  lag_back_project<TI>(h, w.z, front.Z.get(), k, np, M, tau, f.r(), N, w.inv_dev.get(), w.P.get());
  hipLaunchKernelGGL(eeof_sign_norm_kernel, dim3((unsigned)k), dim3(256), 0, h->st, (const double*)w.P.get(), plane, N, N, M, known,
                     w.scale.ensure((size_t)k));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
}

// xmca_extended_eofs on the resident real field of side 0: Gram matrix, lag sum and double centring (csrc/lag_gram.h),
// the k leading eigenvectors of the T' x T' matrix, one back-projection per lag on a row-offset view of the field with 1 / sigma_c
// in the epilogue, sign, and the (M, N_full, k) layout by the transposition and scatter kernels of xmca_get_maps.  Every buffer is
// this call's own: the result of a solve, its vectors and the field planes are only read.
template <typename TI>
void extended_eofs_impl(xmca_handle* h, int M, int tau, int k, const int64_t* keep_idx, int64_t N_full, double* lam_out, double* pcs_out,
                        double* eofs_out) {
  const FieldData<TI>& f = typed<TI>(h).f[0];
  const int T = (int)f.T, np = T - (M - 1) * tau;
  const int64_t N = f.N;
  EeofFront front;
  eeof_leading_vectors<TI>(h, "extended_eofs", M, tau, k, front);
  const std::vector<double>& lam = front.lam;
  DevBuf<double>& Z = front.Z;
  EeofPatterns<TI> pat;
  DevBuf<double> tmp, out;
  DevBuf<int64_t> row_of;
  const int64_t* rows = upload_inverse_map(h, keep_idx, N, N_full, row_of);
  const int64_t plane = (int64_t)k * N;
  eeof_patterns<TI>(h, front, M, tau, k, pat);
  DevBuf<double>& P = pat.P;
  DevBuf<double>& scale = pat.scale;
  h->tm.begin("eeof_assemble");
  const size_t slice = (size_t)N_full * k;
  tmp.ensure((size_t)N * k);
  out.ensure((size_t)M * slice);
  for (int j = 0; j < M; ++j) {
    hipLaunchKernelGGL((eof_transpose_kernel<double, double>), dim3((unsigned)ceil_div(N, (int64_t)32), (unsigned)ceil_div(k, 32)), dim3(256), 0,
                       h->st, (const double*)(P.get() + j * plane), (const double*)nullptr, N, N, k, tmp.get());
    hipLaunchKernelGGL((map_finish_kernel<double>), ew_grid((int64_t)slice), dim3(EW_BLOCK), 0, h->st, (const double*)tmp.get(), 0,
                       rows, N_full, k, (const double*)scale.get(),
                       (const double*)nullptr, (const double*)nullptr, (int)MAP_EOF, 0, out.get() + (size_t)j * slice);
  }
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  std::vector<double> zh((size_t)k * np), sc((size_t)k);
  XMCA_HIP(hipMemcpyAsync(eofs_out, out.get(), sizeof(double) * (size_t)M * slice, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(zh.data(), Z.get(), sizeof(double) * (size_t)k * np, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(sc.data(), scale.get(), sizeof(double) * k, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  // PCs: U sqrt(T' - 1) with the patterns' signs (T' x k values)
  const double root = std::sqrt((double)(np - 1));
  for (int c = 0; c < k; ++c) {
    const double w = sc[(size_t)c] < 0.0 ? -root : root;
    for (int t = 0; t < np; ++t) pcs_out[(size_t)t * k + c] = zh[(size_t)c * np + t] * w;
  }
  std::memcpy(lam_out, lam.data(), sizeof(double) * np);
}

// xmca_extended_reconstruct: the reconstructed component of the n_sel modes `modes` on the T time steps of the
// resident field.  The front of extended_eofs gives the leading eigenvectors; the selected ones are gathered (Z_sel, q x T'), one
// thin GEMM per lag on a row-offset view of the field forms P (row j q + c = Z_sel[c] X_j; the vectors sum to zero, so the
// uncentred windows give the centred product), lag_expand_kernel forms A~ and 1 / c, the window means fill the last M rows of P
// (add_means), and R = diag(1 / c) A~ P runs row block by row block into the finish of xmca_reconstruct.  Every buffer is this
// call's own.
template <typename TI>
void extended_reconstruct_impl(xmca_handle* h, int M, int tau, const int* modes, int q, bool add_means, const int64_t* keep_idx,
                               int64_t N_full, const double* mean, const double* stdv, const double* inv_weight, double* out, bool out_dev) {
  const FieldData<TI>& f = typed<TI>(h).f[0];
  const int T = (int)f.T, np = T - (M - 1) * tau;
  const int64_t N = f.N;
  const int k = modes[q - 1] + 1;
  const int kin = M * (q + (add_means ? 1 : 0));
  EeofFront front;
  eeof_leading_vectors<TI>(h, "extended_reconstruct", M, tau, k, front);
  DevBuf<double> Zsel, A, inv_count, P, part;
  DevBuf<int> sel, table;
  XMCA_HIP(hipMemcpyAsync(sel.ensure((size_t)q), modes, sizeof(int) * q, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));          // (modes is the caller's)
  h->tm.begin("eeof_expand");
  hipLaunchKernelGGL(lag_select_rows_kernel, ew_grid((int64_t)q * np), dim3(EW_BLOCK), 0, h->st, (const double*)front.Z.get(), np,
                     (const int*)sel.get(), q, Zsel.ensure((size_t)q * np));
  XMCA_HIP(hipGetLastError());
  lag_expand(h->st, Zsel.get(), q, np, M, tau, add_means, A.ensure((size_t)T * kin), inv_count.ensure((size_t)T));
  h->tm.end();
  P.ensure((size_t)kin * N);
  Narrow<TI> z;
  h->tm.begin("eeof_project");
  lag_back_project<TI>(h, z, Zsel.get(), q, np, M, tau, f.r(), N, nullptr, P.get());
  h->tm.end();
  if (add_means) {
    h->tm.begin("eeof_window_means");
    lag_window_means<TI>(h->st, f.r(), T, N, M, tau, P.get() + (int64_t)M * q * N, table, part);
    h->tm.end();
  }
  ReconstructTail tail;
  tail.begin(h, T, keep_idx, N, N_full, mean, stdv, inv_weight, out_dev);
  tail.allocate();
  for (int64_t t0 = 0; t0 < T; t0 += tail.rows) {
    const int tb = (int)std::min<int64_t>(tail.rows, T - t0);
    h->tm.begin("eeof_reconstruct");
    GemmOpts o;          // C = diag(1 / c) A~ P (tb x N, K = kin)
    o.row_scale = inv_count.get() + t0;
    gemm<double, double>(h->st, h->gws, A.get() + t0 * kin, kin, P.get(), N, tail.C.get(), N, tb, (int)N, kin, o);
    h->tm.end();
    tail.finish(h, "eeof_reconstruct", t0, tb, out);
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// (tests) xmca_lag_window_means on the resident field of side 0
template <typename TI>
void lag_window_means_impl(xmca_handle* h, int M, int tau, double* means_out) {
  const FieldData<TI>& f = typed<TI>(h).f[0];
  DevBuf<double> means, part;
  DevBuf<int> table;
  h->tm.begin("eeof_window_means");
  lag_window_means<TI>(h->st, f.r(), (int)f.T, f.N, M, tau, means.ensure((size_t)M * f.N), table, part);
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(means_out, means.get(), sizeof(double) * (size_t)M * f.N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// ---- Monte-Carlo SSA test of extended EOFs (csrc/lag_project.h) ---------------------------------------------
// What one xmca_extended_rule_n / xmca_extended_project call keeps on the device: the front and the patterns of
// xmca_extended_eofs, the column scale d, the GEMM's B operand (the unit-norm patterns, times d where asked) and the scratch of
// one projection.  Every buffer is this call's own: the result of a solve, its vectors and the field planes are only read.
template <typename TI>
struct McssaState {
  EeofFront front;
  EeofPatterns<TI> pat;
  DevBuf<double> d, col_part, col_dev, W, Q, part;
  DevBuf<TI> B;
  int T = 0, M = 0, tau = 0, k = 0;
  int64_t N = 0;

  void begin(xmca_handle* h, const char* what, int M_, int tau_, int k_, bool apply_scale) {
    const FieldData<TI>& f = typed<TI>(h).f[0];
    T = (int)f.T; N = f.N; M = M_; tau = tau_; k = k_;
    eeof_leading_vectors<TI>(h, what, M, tau, k, front);
    eeof_patterns<TI>(h, front, M, tau, k, pat);
    h->tm.begin("mcssa_scale");
    lag_column_scale<TI>(h->st, f.r(), T, N, d.ensure((size_t)N), col_part, col_dev);
    const int64_t total = (int64_t)M * k * N;
    hipLaunchKernelGGL((lagp_scale_patterns_kernel<TI>), ew_grid(total), dim3(EW_BLOCK), 0, h->st, (const double*)pat.P.get(),
                       (const double*)pat.scale.get(), (const double*)(apply_scale ? d.get() : nullptr), k, N, total,
                       B.ensure((size_t)total));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    const int np = T - (M - 1) * tau;
    W.ensure((size_t)T * M * k);
    Q.ensure((size_t)np * k);
    part.ensure(lag_project_scratch(np, k));
  }

  // Lambda of the T x N plane R (k values at `out`, on the device), queued on the handle's stream: W = R B^T, then the shift sum,
  // the centring and the squares
  void project(xmca_handle* h, const TI* R, double* out) {
    h->tm.begin("mcssa_gemm");
    GemmOpts o;
    o.a_kfast = true; o.b_nfast = false;
    gemm<TI, double>(h->st, h->gws, R, N, (const TI*)B.get(), N, W.get(), (int64_t)M * k, T, M * k, (int)N, o);
    h->tm.end();
    h->tm.begin("mcssa_project");
    lag_project(h->st, W.get(), T, M, tau, k, Q.get(), part.get(), out);
    h->tm.end();
  }
};

// xmca_extended_rule_n: runs [run_begin, run_end) of the test.  phi: N values on the host, checked by the caller.
template <typename TI>
void extended_rule_n_impl(xmca_handle* h, int M, int tau, int k, const double* phi, int64_t run_begin, int64_t run_end, uint64_t seed,
                          double* lam_out, double* scale_out, double* surrogates_out) {
  McssaState<TI> s;
  s.begin(h, "extended_rule_n", M, tau, k, true);
  const int64_t n_runs = run_end - run_begin, n = (int64_t)s.T * s.N;
  DevBuf<TI> R;
  DevBuf<double> phi_dev, carry, lam_dev;
  XMCA_HIP(hipMemcpyAsync(phi_dev.ensure((size_t)s.N), phi, sizeof(double) * s.N, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));          // (phi is the caller's)
  if (n_runs > 0) {
    R.ensure((size_t)n);
    lam_dev.ensure((size_t)(n_runs * k));
  }
  for (int64_t r = 0; r < n_runs; ++r) {
    h->tm.begin("mcssa_surrogate");
    hipLaunchKernelGGL((philox_normal_kernel<TI>), ew_grid((n + 1) / 2), dim3(EW_BLOCK), 0, h->st, R.get(), n, seed,
                       (uint32_t)(run_begin + r), (uint32_t)0);
    ar1_filter<TI>(h->st, R.get(), s.T, s.N, phi_dev.get(), carry);
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    s.project(h, R.get(), lam_dev.get() + r * k);
  }
  if (n_runs > 0)
    XMCA_HIP(hipMemcpyAsync(surrogates_out, lam_dev.get(), sizeof(double) * (size_t)(n_runs * k), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(scale_out, s.d.get(), sizeof(double) * (size_t)s.N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  std::memcpy(lam_out, s.front.lam.data(), sizeof(double) * (size_t)(s.T - (M - 1) * tau));
}

// (tests) xmca_extended_project: the same front, scale, GEMM and projection kernels on a field of the caller's
template <typename TI>
void extended_project_impl(xmca_handle* h, int M, int tau, int k, const double* R_host, bool apply_scale, double* out) {
  McssaState<TI> s;
  s.begin(h, "extended_project", M, tau, k, apply_scale);
  const size_t n = (size_t)s.T * (size_t)s.N;
  HostPlanes<TI> R;
  DevBuf<double> lam_dev;
  upload_planes<TI>(h, R_host, n, false, R);
  s.project(h, R.r, lam_dev.ensure((size_t)k));
  XMCA_HIP(hipMemcpyAsync(out, lam_dev.get(), sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// (tests) xmca_lag_project: the projection kernels alone on a host matrix
inline void lag_project_impl(xmca_handle* h, const double* W_host, int T, int M, int tau, int k, double* out) {
  const int np = T - (M - 1) * tau;
  const size_t nw = (size_t)T * M * k;
  DevBuf<double> W, Q, part, lam_dev;
  XMCA_HIP(hipMemcpyAsync(W.ensure(nw), W_host, sizeof(double) * nw, hipMemcpyHostToDevice, h->st));
  h->tm.begin("mcssa_project");
  lag_project(h->st, W.get(), T, M, tau, k, Q.ensure((size_t)np * k), part.ensure(lag_project_scratch(np, k)), lam_dev.ensure((size_t)k));
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(out, lam_dev.get(), sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// ---- DINEOF gap filling (csrc/gap_fill.h) ----------------------------------------------------------------------
// The host checks of a field with gaps, before anything is launched: no Inf, a finite value in every column.  Returns the number
// of present entries.
template <typename TI>
int64_t gap_check_field(const std::string& what, const TI* X, int64_t T, int64_t N) {
  std::vector<unsigned char> seen((size_t)N, 0);
  int64_t present = 0;
  bool inf = false;
  for (int64_t t = 0; t < T; ++t) {
    const TI* row = X + t * N;
    for (int64_t n = 0; n < N; ++n) {
      const TI v = row[n];
      if (v == v) { inf = inf || std::isinf(v); seen[(size_t)n] = 1; ++present; }
    }
  }
  XMCA_CHECK(!inf, XMCA_ERR_INVALID, what + ": the field holds an Inf (NaN marks a missing value)");
  for (int64_t n = 0; n < N; ++n) XMCA_CHECK(seen[(size_t)n], XMCA_ERR_INVALID, what + ": a column has no finite value (set it aside first)");
  return present;
}

// ... and of the withheld entries: flat indices of present entries, each once
template <typename TI>
void gap_check_withheld(const TI* X, int64_t total, const int64_t* cv_idx, int64_t n_cv) {
  std::vector<int64_t> sorted(cv_idx, cv_idx + n_cv);
  std::sort(sorted.begin(), sorted.end());
  for (int64_t i = 0; i < n_cv; ++i) {
    const int64_t e = sorted[(size_t)i];
    XMCA_CHECK(e >= 0 && e < total, XMCA_ERR_INVALID, "fill_gaps: a cross-validation index is out of range");
    XMCA_CHECK(i == 0 || e != sorted[(size_t)i - 1], XMCA_ERR_INVALID, "fill_gaps: a cross-validation index is repeated");
    XMCA_CHECK(X[e] == X[e], XMCA_ERR_INVALID, "fill_gaps: a cross-validation index points at a missing value");
  }
}

// xmca_fill_gaps, xmca_fill_gaps_lagged: the raw plane stays on the device and only its missing entries are written at the end, so
// present entries come back with their bits.  One iteration is the Gram product G of the working plane A, the k leading
// eigenvectors Z of K, P = Z A on the M lagged views of A and the fill kernel; the change d_i comes back to the host after every
// iteration (the eigensolver has synchronised the stream before).  M = 1 (DINEOF): K is G itself and the fill is
// gap_fill_kernel.  M > 1 (M-SSA gap filling): K is the lag sum of G (csrc/lag_gram.h, not centred), T' x T' with
// T' = T - (M - 1) tau, and the fill is the diagonally averaged gap_lag_fill_kernel.  The eigensolver's route, the Z plane and
// the polish are all taken at T'.  Every buffer is this call's own.
template <typename TI>
void fill_gaps_impl(xmca_handle* h, const TI* X, int T, int64_t N, int64_t n_present, const int64_t* cv_idx, int64_t n_cv, int k, int M, int tau,
                    int max_iter, double tol, TI* out, double* history_out, int* iters_out, double* cv_rms_out, double* lam_out) {
  const size_t total = (size_t)T * N;
  const int Tp = T - (M - 1) * tau;
  const int64_t tiles = gap_fill_tiles(T, N);
  DevBuf<TI> raw, A, saved;
  DevBuf<unsigned char> mask;
  DevBuf<double> mean, stat, part, P, Z, lam_dev, hist, cv, W, S, Zp, K, lag_part, lag_mean;
  DevBuf<int64_t> idx;
  GapCenterScratch scratch;
  CPlanes G;
  Narrow<TI> z;
  XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  h->tm.begin("gap_center");
  gap_center<TI>(h->st, raw.get(), T, N, A.ensure(total), mask.ensure(total), mean.ensure((size_t)N), stat.ensure(2), scratch);
  if (n_cv > 0) {
    XMCA_HIP(hipMemcpyAsync(idx.ensure((size_t)n_cv), cv_idx, sizeof(int64_t) * n_cv, hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL((gap_withhold_kernel<TI>), ew_grid(n_cv), dim3(EW_BLOCK), 0, h->st, A.get(), mask.get(), (const int64_t*)idx.get(), n_cv,
                       saved.ensure((size_t)n_cv));
    XMCA_HIP(hipGetLastError());
  }
  h->tm.end();
  double stat_host[2] = {0.0, 0.0};
  XMCA_HIP(hipMemcpyAsync(stat_host, stat.get(), sizeof(stat_host), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  XMCA_CHECK(std::isfinite(stat_host[0]) && stat_host[0] > 0.0, XMCA_ERR_NUMERIC, "fill_gaps: the present values have no variance about their column means");
  const double n_masked = (double)((int64_t)total - n_present + n_cv);
  FieldData<TI> f;          // the working plane as a field of the solver's Gram product
  f.T = T;
  f.N = N;
  f.ext_re = A.get();
  Solver<TI> s(h->st, h->gws, h->ews, h->tm);
  std::vector<double> lam;
  P.ensure((size_t)M * k * N);
  if (M > 1) K.ensure((size_t)Tp * Tp);
  // Where the eigensolver takes the block Jacobi sweeps it forms all T' vectors whatever is asked for: they are all taken, and the
  // leading k are polished against the others (csrc/gap_fill.h).  On the tridiagonal route the partial stage gives the leading k
  // alone and nothing is polished.  Not covered: a problem that the partial stage hands back to the sweeps (bit-equal leading
  // eigenvalues, a refused clean-up) comes back as k unpolished Jacobi vectors.
  const bool polish = !evd_vectors_by_reduction(Tp, false);
  Z.ensure((size_t)(polish ? Tp : k) * Tp);
  if (polish) { W.ensure((size_t)k * Tp); S.ensure((size_t)k * Tp); Zp.ensure((size_t)k * Tp); }
  lam_dev.ensure((size_t)Tp);
  part.ensure((size_t)tiles);
  hist.ensure((size_t)max_iter);
  int iters = 0;
  for (int i = 0; i < max_iter; ++i) {
    s.gram(f, false, G);
    const double* Km = G.r();
    if (M > 1) {
      h->tm.begin("gap_lag_gram");
      lag_gram(h->st, G.r(), T, T, M, tau, false, K.get(), lag_part, lag_mean);
      h->tm.end();
      Km = K.get();
    }
    EvdInfo info;
    h->tm.begin("gap_eigh");
    hermitian_evd(h->st, h->ews, Km, nullptr, Tp, Tp, lam, lam_dev.get(), Z.get(), nullptr, Tp, &info, false, polish ? -1 : k);
    XMCA_HIP(hipStreamSynchronize(h->st));
    const bool usable = std::isfinite(lam[0]) && lam[0] > 0.0;
    const double* Zk = Z.get();
    if (polish && usable) {         // (csrc/gap_fill.h gap_polish_coeff_kernel) S = (Z_k K) Z^T, O = Z_k Z^T, coefficients, Z_k += C Z
      GemmOpts o;
      gemm<double, double>(h->st, h->gws, (const double*)Z.get(), Tp, Km, Tp, W.get(), Tp, k, Tp, Tp, o);
      o.b_nfast = false;
      gemm<double, double>(h->st, h->gws, (const double*)W.get(), Tp, (const double*)Z.get(), Tp, S.get(), Tp, k, Tp, Tp, o);
      gemm<double, double>(h->st, h->gws, (const double*)Z.get(), Tp, (const double*)Z.get(), Tp, W.get(), Tp, k, Tp, Tp, o);
      hipLaunchKernelGGL(gap_polish_coeff_kernel, ew_grid((int64_t)k * Tp), dim3(EW_BLOCK), 0, h->st, S.get(), (const double*)W.get(),
                         (const double*)lam_dev.get(), k, Tp);
      XMCA_HIP(hipGetLastError());
      XMCA_HIP(hipMemcpyAsync(Zp.get(), Z.get(), sizeof(double) * (size_t)k * Tp, hipMemcpyDeviceToDevice, h->st));
      o.b_nfast = true;
      o.beta = 1.0;
      gemm<double, double>(h->st, h->gws, (const double*)S.get(), Tp, (const double*)Z.get(), Tp, Zp.get(), Tp, k, Tp, Tp, o);
      Zk = Zp.get();
    }
    h->tm.end();
    XMCA_CHECK(usable, XMCA_ERR_NUMERIC, "fill_gaps: the iterate has no variance");
    h->tm.begin("gap_project");
    lag_back_project<TI>(h, z, Zk, k, Tp, M, tau, (const TI*)A.get(), N, nullptr, P.get());
    h->tm.end();
    h->tm.begin("gap_fill");
    if (M == 1) gap_fill_step<TI>(h->st, A.get(), mask.get(), Zk, P.get(), T, N, k, part.get());
    else gap_lag_fill_step<TI>(h->st, A.get(), mask.get(), Zk, P.get(), T, N, k, M, tau, part.get());
    hipLaunchKernelGGL(gap_change_kernel, dim3(1), dim3(256), 0, h->st, (const double*)part.get(), tiles, n_masked, (const double*)stat.get(),
                       hist.get() + i, (double*)nullptr);
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    XMCA_HIP(hipMemcpyAsync(history_out + i, hist.get() + i, sizeof(double), hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
    iters = i + 1;
    if (history_out[i] < tol) break;
  }
  h->tm.begin("gap_finish");
  if (n_cv > 0)
    hipLaunchKernelGGL((gap_cv_rms_kernel<TI>), dim3(1), dim3(256), 0, h->st, (const TI*)A.get(), (const int64_t*)idx.get(), (const TI*)saved.get(),
                       n_cv, cv.ensure(1));
  hipLaunchKernelGGL((gap_finish_kernel<TI>), ew_grid((int64_t)total), dim3(EW_BLOCK), 0, h->st, raw.get(), (const TI*)A.get(),
                     (const unsigned char*)mask.get(), (const double*)mean.get(), N, (int64_t)total);
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  *cv_rms_out = std::nan("");
  if (n_cv > 0) XMCA_HIP(hipMemcpyAsync(cv_rms_out, cv.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(out, raw.get(), sizeof(TI) * total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  *iters_out = iters;
  std::memcpy(lam_out, lam.data(), sizeof(double) * (size_t)k);
}

// (tests) xmca_gap_center: the centring and mask kernels alone
template <typename TI>
void gap_center_impl(xmca_handle* h, const TI* X, int T, int64_t N, double* mean_out, unsigned char* mask_out, double* A_out, double* scale_out) {
  const size_t total = (size_t)T * N;
  DevBuf<TI> raw, A;
  DevBuf<unsigned char> mask;
  DevBuf<double> mean, stat, wide;
  GapCenterScratch scratch;
  XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  h->tm.begin("gap_center");
  gap_center<TI>(h->st, raw.get(), T, N, A.ensure(total), mask.ensure(total), mean.ensure((size_t)N), stat.ensure(2), scratch);
  h->tm.end();
  hipLaunchKernelGGL((convert_kernel<TI, double>), ew_grid((int64_t)total), dim3(EW_BLOCK), 0, h->st, (const TI*)A.get(), wide.ensure(total),
                     (int64_t)total);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(mean_out, mean.get(), sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(mask_out, mask.get(), total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(A_out, wide.get(), sizeof(double) * total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(scale_out, stat.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// (tests) xmca_gap_fill_step: the fill kernel and the finish of its partial sums alone
template <typename TI>
void gap_fill_step_impl(xmca_handle* h, const TI* A_in, const unsigned char* mask_in, const double* Z_in, const double* P_in, int T, int64_t N,
                        int k, TI* A_out, double* sum_out) {
  const size_t total = (size_t)T * N;
  const int64_t tiles = gap_fill_tiles(T, N);
  DevBuf<TI> A;
  DevBuf<unsigned char> mask;
  DevBuf<double> Z, P, part, sum;
  XMCA_HIP(hipMemcpyAsync(A.ensure(total), A_in, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(mask.ensure(total), mask_in, total, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Z.ensure((size_t)k * T), Z_in, sizeof(double) * (size_t)k * T, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(P.ensure((size_t)k * N), P_in, sizeof(double) * (size_t)k * N, hipMemcpyHostToDevice, h->st));
  h->tm.begin("gap_fill");
  gap_fill_step<TI>(h->st, A.get(), mask.get(), Z.get(), P.get(), T, N, k, part.ensure((size_t)tiles));
  hipLaunchKernelGGL(gap_change_kernel, dim3(1), dim3(256), 0, h->st, (const double*)part.get(), tiles, 0.0, (const double*)nullptr,
                     (double*)nullptr, sum.ensure(1));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(A_out, A.get(), sizeof(TI) * total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(sum_out, sum.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// (tests) xmca_gap_lag_fill_step: the lagged fill kernel and the finish of its partial sums alone; Z k x T', P M k x N
template <typename TI>
void gap_lag_fill_step_impl(xmca_handle* h, const TI* A_in, const unsigned char* mask_in, const double* Z_in, const double* P_in, int T,
                            int64_t N, int k, int M, int tau, TI* A_out, double* sum_out) {
  const size_t total = (size_t)T * N, nz = (size_t)k * (size_t)(T - (M - 1) * tau), np = (size_t)M * k * N;
  const int64_t tiles = gap_fill_tiles(T, N);
  DevBuf<TI> A;
  DevBuf<unsigned char> mask;
  DevBuf<double> Z, P, part, sum;
  XMCA_HIP(hipMemcpyAsync(A.ensure(total), A_in, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(mask.ensure(total), mask_in, total, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Z.ensure(nz), Z_in, sizeof(double) * nz, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(P.ensure(np), P_in, sizeof(double) * np, hipMemcpyHostToDevice, h->st));
  h->tm.begin("gap_fill");
  gap_lag_fill_step<TI>(h->st, A.get(), mask.get(), Z.get(), P.get(), T, N, k, M, tau, part.ensure((size_t)tiles));
  hipLaunchKernelGGL(gap_change_kernel, dim3(1), dim3(256), 0, h->st, (const double*)part.get(), tiles, 0.0, (const double*)nullptr,
                     (double*)nullptr, sum.ensure(1));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(A_out, A.get(), sizeof(TI) * total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(sum_out, sum.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// xmca_column_regress, xmca_column_residual: the field comes from the host or - through the copy kernels of
// xmca_set_field_strided - from the caller's device memory into a buffer of this call; the mask / widen pass; with coef_in == nullptr
// the fit - right-hand sides B^T X0 (k x N) and, where an entry is missing, the packed normal matrices and the counts
// Q^T P ((k (k + 1) / 2 + 1) x N: the pair products of the basis columns and a row of ones against the presence plane) by the
// GEMM, one shared normal matrix summed on the host where nothing is missing, then the solve kernel - else the given coefficients
// (a column with a NaN among them counts as not fitted); the residual pass, into the caller's device memory or a buffer that is
// copied to the host.  Every buffer is this call's own.
template <typename TI>
void column_regress_impl(xmca_handle* h, const void* X, bool in_device, int T, int64_t N, int64_t stride_t, int64_t stride_n, const double* basis,
                         int k, const double* coef_in, TI* out, bool out_device, double* coef_out, unsigned char* fitted_out) {
  const size_t total = (size_t)T * N;
  const int m = reg_packed(k);
  const bool fit = coef_in == nullptr;
  DevBuf<TI> raw;
  DevBuf<unsigned char> mask, fitted;
  DevBuf<double> wide, pres, Bd, Ad, rhs, nm, coef;
  RegMaskScratch scratch;
  if (in_device) {
    h->tm.begin("ingest_strided");
    ingest_strided<TI>(h->st, static_cast<const TI*>(X), T, N, stride_t, stride_n, raw.ensure(total));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  } else {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  }
  XMCA_HIP(hipMemcpyAsync(Bd.ensure((size_t)T * k), basis, sizeof(double) * (size_t)T * k, hipMemcpyHostToDevice, h->st));
  h->tm.begin("reg_mask");
  reg_mask<TI>(h->st, raw.get(), (int64_t)total, mask.ensure(total), wide.ensure(total), fit ? pres.ensure(total) : nullptr, scratch);
  h->tm.end();
  coef.ensure((size_t)k * N);
  fitted.ensure((size_t)N);
  std::vector<unsigned char> fitted_host;
  std::vector<double> a_host, shared;
  if (fit) {
    // rows 0 .. k-1: B^T; rows k .. k+m-1: the pair products b_i b_j in packed order; row k+m: ones (the count)
    a_host.resize((size_t)(k + m + 1) * T);
    for (int t = 0; t < T; ++t) {
      const double* b = basis + (size_t)t * k;
      for (int i = 0; i < k; ++i) {
        a_host[(size_t)i * T + t] = b[i];
        for (int j = 0; j <= i; ++j) a_host[(size_t)(k + i * (i + 1) / 2 + j) * T + t] = b[i] * b[j];
      }
      a_host[(size_t)(k + m) * T + t] = 1.0;
    }
    XMCA_HIP(hipMemcpyAsync(Ad.ensure(a_host.size()), a_host.data(), sizeof(double) * a_host.size(), hipMemcpyHostToDevice, h->st));
    double missing = 0.0;
    XMCA_HIP(hipMemcpyAsync(&missing, scratch.count.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
    h->tm.begin("reg_moments");
    GemmOpts o;
    gemm<double, double>(h->st, h->gws, (const double*)Ad.get(), T, (const double*)wide.get(), N, rhs.ensure((size_t)k * N), N, k, (int)N, T, o);
    int64_t es = N, ns = 1;
    if (missing > 0.0) {
      gemm<double, double>(h->st, h->gws, (const double*)Ad.get() + (size_t)k * T, T, (const double*)pres.get(), N, nm.ensure((size_t)(m + 1) * N),
                           N, m + 1, (int)N, T, o);
    } else {          // one normal matrix for every column: the rows of a_host summed over t, ascending
      shared.assign((size_t)m + 1, 0.0);
      for (int e = 0; e <= m; ++e) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += a_host[(size_t)(k + e) * T + t];
        shared[(size_t)e] = s;
      }
      XMCA_HIP(hipMemcpyAsync(nm.ensure((size_t)m + 1), shared.data(), sizeof(double) * ((size_t)m + 1), hipMemcpyHostToDevice, h->st));
      es = 1;
      ns = 0;
    }
    h->tm.end();
    h->tm.begin("reg_solve");
    reg_solve(h->st, k, nm.get(), es, ns, rhs.get(), N, coef.get(), fitted.get());
    h->tm.end();
    XMCA_HIP(hipMemcpyAsync(coef_out, coef.get(), sizeof(double) * (size_t)k * N, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(fitted_out, fitted.get(), (size_t)N, hipMemcpyDeviceToHost, h->st));
  } else {
    fitted_host.assign((size_t)N, 1);
    for (int c = 0; c < k; ++c)
      for (int64_t n = 0; n < N; ++n)
        if (!(coef_in[(size_t)c * N + n] == coef_in[(size_t)c * N + n])) fitted_host[(size_t)n] = 0;
    XMCA_HIP(hipMemcpyAsync(coef.get(), coef_in, sizeof(double) * (size_t)k * N, hipMemcpyHostToDevice, h->st));
    XMCA_HIP(hipMemcpyAsync(fitted.get(), fitted_host.data(), (size_t)N, hipMemcpyHostToDevice, h->st));
  }
  h->tm.begin("reg_residual");
  TI* dst = out_device ? out : raw.get();          // (the raw plane has been read: the mask pass is ahead on the stream)
  reg_residual<TI>(h->st, wide.get(), mask.get(), Bd.get(), coef.get(), fitted.get(), T, N, k, dst);
  h->tm.end();
  if (!out_device) XMCA_HIP(hipMemcpyAsync(out, raw.get(), sizeof(TI) * total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// xmca_time_filter: the field comes from the host or - through the copy kernels of xmca_set_field_strided - from
// the caller's device memory into a buffer of this call; the one filter kernel writes the caller's device memory, or a buffer
// that is copied to the host.  Every buffer is this call's own.
template <typename TI>
void time_filter_impl(xmca_handle* h, const void* X, bool in_device, int T, int64_t N, int64_t stride_t, int64_t stride_n, const double* weights,
                      int L, bool complement, bool renormalise, double den_min, bool trim, TI* out, bool out_device) {
  const size_t total = (size_t)T * N;
  const size_t total_out = (size_t)(trim ? T - (L - 1) : T) * N;
  DevBuf<TI> raw, res;
  DevBuf<double> wd;
  if (in_device) {
    h->tm.begin("ingest_strided");
    ingest_strided<TI>(h->st, static_cast<const TI*>(X), T, N, stride_t, stride_n, raw.ensure(total));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  } else {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  }
  XMCA_HIP(hipMemcpyAsync(wd.ensure((size_t)L), weights, sizeof(double) * (size_t)L, hipMemcpyHostToDevice, h->st));
  TI* dst = out_device ? out : res.ensure(total_out);
  h->tm.begin("time_filter");
  time_filter<TI>(h->st, raw.get(), T, N, wd.get(), L, complement, renormalise, den_min, trim, dst);
  h->tm.end();
  if (!out_device) XMCA_HIP(hipMemcpyAsync(out, res.get(), sizeof(TI) * total_out, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// xmca_lead_lag_maps: the field comes from the host or - through the copy kernels of xmca_set_field_strided - from
// the caller's device memory into a buffer of this call; the centring pass, the lag-1 pass (Bretherton), the moment kernel into a
// moments plane of this call, the finish into the caller's device memory or into buffers that are copied to the host.  Every
// buffer is this call's own.
template <typename TI>
void lead_lag_impl(xmca_handle* h, const void* X, bool in_device, int T, int64_t N, int64_t stride_t, int64_t stride_n, const double* Y, int q,
                   const int* lags, int n_lags, int min_pairs, bool bretherton, const double* rho_y, TI* r_out, TI* slope_out, double* p_out,
                   int* dof_out, int* pairs_out, double* lag1_out, bool out_device) {
  const size_t total = (size_t)T * N;
  const size_t planes = (size_t)n_lags * N, entries = planes * q;
  DevBuf<TI> raw, rd, sd;
  DevBuf<double> cn, Yd, rx, ry, mom, ln, pd;
  DevBuf<int> n0, lg, dd, prs;
  if (in_device) {
    h->tm.begin("ingest_strided");
    ingest_strided<TI>(h->st, static_cast<const TI*>(X), T, N, stride_t, stride_n, raw.ensure(total));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  } else {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  }
  std::vector<double> table((size_t)T + 1, 0.0);          // log_norm[k] at 3 <= k <= T: a dof never exceeds a pair count, and that not T
  for (int k = 3; k <= T; ++k) table[(size_t)k] = pvalue_log_norm(k);
  XMCA_HIP(hipMemcpyAsync(Yd.ensure((size_t)T * q), Y, sizeof(double) * (size_t)T * q, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(lg.ensure((size_t)n_lags), lags, sizeof(int) * (size_t)n_lags, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(ln.ensure(table.size()), table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, h->st));
  if (bretherton) XMCA_HIP(hipMemcpyAsync(ry.ensure((size_t)q), rho_y, sizeof(double) * (size_t)q, hipMemcpyHostToDevice, h->st));
  const dim3 cols((unsigned)ceil_div(N, LL_COLS)), block(LL_COLS);
  h->tm.begin("lead_lag_center");
  hipLaunchKernelGGL((lead_lag_center_kernel<TI>), cols, block, 0, h->st, (const TI*)raw.get(), T, N, cn.ensure((size_t)N), n0.ensure((size_t)N));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  double* rho_x = nullptr;
  if (bretherton) {
    rho_x = out_device ? lag1_out : rx.ensure((size_t)N);
    h->tm.begin("lead_lag_lag1");
    hipLaunchKernelGGL((lag1_gappy_kernel<TI>), cols, block, 0, h->st, (const TI*)raw.get(), T, N, (const double*)cn.get(), (const int*)n0.get(),
                       rho_x);
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  }
  int* pairs = out_device ? pairs_out : prs.ensure(planes);
  h->tm.begin("lead_lag_moments");
  lead_lag_moments<TI>(h->st, raw.get(), T, N, cn.get(), Yd.get(), q, lg.get(), n_lags, pairs, mom.ensure(planes * (size_t)ll_moments(q)));
  h->tm.end();
  h->tm.begin("lead_lag_finish");
  hipLaunchKernelGGL((lead_lag_finish_kernel<TI>), ew_grid((int64_t)entries), dim3(EW_BLOCK), 0, h->st, (const int*)pairs, (const double*)mom.get(),
                     N, q, n_lags, min_pairs, (const double*)rho_x, (const double*)(bretherton ? ry.get() : nullptr), (const double*)ln.get(),
                     out_device ? r_out : rd.ensure(entries), out_device ? slope_out : sd.ensure(entries),
                     out_device ? p_out : pd.ensure(entries), out_device ? dof_out : dd.ensure(entries));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  if (!out_device) {
    XMCA_HIP(hipMemcpyAsync(r_out, rd.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(slope_out, sd.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(p_out, pd.get(), sizeof(double) * entries, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(dof_out, dd.get(), sizeof(int) * entries, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(pairs_out, prs.get(), sizeof(int) * planes, hipMemcpyDeviceToHost, h->st));
    if (bretherton) XMCA_HIP(hipMemcpyAsync(lag1_out, rx.get(), sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, h->st));
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// xmca_spectral_maps: the field comes from the host or - through the copy kernels of xmca_set_field_strided - from
// the caller's device memory into a buffer of this call; the host tables (twiddles, DFT of the weights, effective segments); the
// centring pass (detrend = mean), the index spectra, the segment kernel into a sums plane of this call, the finish into the
// caller's device memory or into buffers that are copied to the host.  Every buffer is this call's own.
template <typename TI>
void spectral_impl(xmca_handle* h, const void* X, bool in_device, int T, int64_t N, int64_t stride_t, int64_t stride_n, const double* Y, int q, int L,
                   int step, const double* weights, bool demean, const int* bins, int F, double fs, int min_segments, TI* power_out,
                   TI* ipower_out, TI* co_out, TI* quad_out, TI* coh_out, TI* phase_out, TI* gain_out, double* p_out, int* seg_out,
                   bool out_device) {
  const size_t total = (size_t)T * N;
  const int K = (T - L) / step + 1;
  const size_t planes = (size_t)F * N, entries = planes * (size_t)q;
  std::vector<double> tw, W, Ke;
  double w2 = 0.0;
  sp_tables(weights, L, step, bins, F, K, tw, W, &w2, Ke);
  DevBuf<TI> raw, o_pw, o_ip, o_co, o_qu, o_ch, o_ph, o_ga;
  DevBuf<double> cn, Yd, twd, wd, Wd, Ked, Ys, ey, sums, rr, pd;
  DevBuf<int> n0, bd, sg;
  if (in_device) {
    h->tm.begin("ingest_strided");
    ingest_strided<TI>(h->st, static_cast<const TI*>(X), T, N, stride_t, stride_n, raw.ensure(total));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  } else {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(total), X, sizeof(TI) * total, hipMemcpyHostToDevice, h->st));
  }
  XMCA_HIP(hipMemcpyAsync(twd.ensure(tw.size()), tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(wd.ensure((size_t)L), weights, sizeof(double) * (size_t)L, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Wd.ensure(W.size()), W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Ked.ensure(Ke.size()), Ke.data(), sizeof(double) * Ke.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(bd.ensure((size_t)F), bins, sizeof(int) * (size_t)F, hipMemcpyHostToDevice, h->st));
  const double2* tw_d = reinterpret_cast<const double2*>(twd.get());
  const double2* W_d = reinterpret_cast<const double2*>(Wd.get());
  cn.ensure((size_t)N);
  if (demean) {
    h->tm.begin("spectral_center");
    hipLaunchKernelGGL((lead_lag_center_kernel<TI>), dim3((unsigned)ceil_div(N, LL_COLS)), dim3(LL_COLS), 0, h->st, (const TI*)raw.get(), T, N, cn.get(),
                       n0.ensure((size_t)N));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
  } else {
    XMCA_HIP(hipMemsetAsync(cn.get(), 0, sizeof(double) * (size_t)N, h->st));
  }
  const double2* Y_d = nullptr;
  if (q > 0) {
    XMCA_HIP(hipMemcpyAsync(Yd.ensure((size_t)T * q), Y, sizeof(double) * (size_t)T * q, hipMemcpyHostToDevice, h->st));
    h->tm.begin("spectral_index");
    spectral_index(h->st, Yd.get(), q, L, step, K, demean ? 1 : 0, tw_d, wd.get(), w2, bd.get(), W_d, F,
                   reinterpret_cast<double2*>(Ys.ensure(2 * (size_t)K * F * q)), ey.ensure((size_t)K * q));
    h->tm.end();
    Y_d = reinterpret_cast<const double2*>(Ys.get());
  }
  int* seg = out_device ? seg_out : sg.ensure((size_t)N);
  h->tm.begin("spectral_segments");
  spectral_segments<TI>(h->st, raw.get(), N, cn.get(), q, L, step, K, demean ? 1 : 0, tw_d, wd.get(), w2, bd.get(), W_d, F, Y_d,
                        q > 0 ? ey.get() : nullptr, sums.ensure(planes * (size_t)sp_sums(q)), seg, rr.ensure((size_t)N * (1 + q)));
  h->tm.end();
  h->tm.begin("spectral_finish");
  hipLaunchKernelGGL((spectral_finish_kernel<TI>), ew_grid((int64_t)(planes * (size_t)(q > 0 ? q : 1))), dim3(EW_BLOCK), 0, h->st,
                     (const double*)sums.get(), (const int*)seg, (const double*)rr.get(), (const double*)Ked.get(), (const int*)bd.get(), N, q, F, L, fs,
                     w2, min_segments, out_device ? power_out : o_pw.ensure(planes),
                     q == 0 ? nullptr : (out_device ? ipower_out : o_ip.ensure(entries)), q == 0 ? nullptr : (out_device ? co_out : o_co.ensure(entries)),
                     q == 0 ? nullptr : (out_device ? quad_out : o_qu.ensure(entries)), q == 0 ? nullptr : (out_device ? coh_out : o_ch.ensure(entries)),
                     q == 0 ? nullptr : (out_device ? phase_out : o_ph.ensure(entries)), q == 0 ? nullptr : (out_device ? gain_out : o_ga.ensure(entries)),
                     q == 0 ? nullptr : (out_device ? p_out : pd.ensure(entries)));
  XMCA_HIP(hipGetLastError());
  h->tm.end();
  if (!out_device) {
    XMCA_HIP(hipMemcpyAsync(power_out, o_pw.get(), sizeof(TI) * planes, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipMemcpyAsync(seg_out, sg.get(), sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, h->st));
    if (q > 0) {
      XMCA_HIP(hipMemcpyAsync(ipower_out, o_ip.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(co_out, o_co.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(quad_out, o_qu.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(coh_out, o_ch.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(phase_out, o_ph.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(gain_out, o_ga.get(), sizeof(TI) * entries, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipMemcpyAsync(p_out, pd.get(), sizeof(double) * entries, hipMemcpyDeviceToHost, h->st));
    }
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// (tests) xmca_reg_mask: the mask / widen pass alone
template <typename TI>
void reg_mask_impl(xmca_handle* h, const TI* X, int64_t total, unsigned char* mask_out, double* wide_out, int64_t* missing_out) {
  DevBuf<TI> raw;
  DevBuf<unsigned char> mask;
  DevBuf<double> wide;
  RegMaskScratch scratch;
  XMCA_HIP(hipMemcpyAsync(raw.ensure((size_t)total), X, sizeof(TI) * (size_t)total, hipMemcpyHostToDevice, h->st));
  h->tm.begin("reg_mask");
  reg_mask<TI>(h->st, raw.get(), total, mask.ensure((size_t)total), wide.ensure((size_t)total), (double*)nullptr, scratch);
  h->tm.end();
  double missing = 0.0;
  XMCA_HIP(hipMemcpyAsync(mask_out, mask.get(), (size_t)total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(wide_out, wide.get(), sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(&missing, scratch.count.get(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  *missing_out = (int64_t)missing;
}

// (tests) xmca_reg_solve: the solve kernel alone on host moments
void reg_solve_impl(xmca_handle* h, const double* normal, bool shared, const double* rhs_in, int64_t N, int k, double* coef_out,
                    unsigned char* fitted_out) {
  const size_t n_nm = (size_t)(reg_packed(k) + 1) * (shared ? 1 : (size_t)N);
  DevBuf<double> nm, rhs, coef;
  DevBuf<unsigned char> fitted;
  XMCA_HIP(hipMemcpyAsync(nm.ensure(n_nm), normal, sizeof(double) * n_nm, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(rhs.ensure((size_t)k * N), rhs_in, sizeof(double) * (size_t)k * N, hipMemcpyHostToDevice, h->st));
  h->tm.begin("reg_solve");
  reg_solve(h->st, k, nm.get(), shared ? 1 : N, shared ? 0 : 1, rhs.get(), N, coef.ensure((size_t)k * N), fitted.ensure((size_t)N));
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(coef_out, coef.get(), sizeof(double) * (size_t)k * N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(fitted_out, fitted.get(), (size_t)N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// ---- bootstrapping: working copies on the device -----------------------------------------------------------------
template <typename TI>
void bootstrap_begin_impl(xmca_handle* h, int n_fields) {
  TypedState<TI>& ts = typed<TI>(h);
  h->boot_T = ts.f[0].T;
  h->boot_fields = n_fields;
  for (int s = 0; s < n_fields; ++s) {
    XMCA_CHECK(h->field_set[s] && ts.f[s].T == h->boot_T, XMCA_ERR_STATE, "bootstrap: set the fields first (same number of time steps)");
    h->boot_N[s] = ts.f[s].N;
    const size_t n = (size_t)ts.f[s].T * ts.f[s].N;
    XMCA_HIP(hipMemcpyAsync(ts.boot[s].ensure(n), ts.f[s].r(), sizeof(TI) * n, hipMemcpyDeviceToDevice, h->st));
  }
  XMCA_HIP(hipStreamSynchronize(h->st));
}

// The replicates of a bootstrap: rows (axis 0) or columns (axis 1) of the ORIGINAL working copies (xmca_bootstrap_begin) are
// gathered through the composed index of replicate r - the reference's cumulative resampling X <- X[idx_r] unrolled on the host,
// c_r = c_{r-1}[idx_r] - so the replicates do not depend on each other on the device and can run in lanes.  Row indices address
// the T rows of a side's own copy; column indices address the columns of [left | right], Nl + Nr of them (the reference
// resamples the concatenation when both sides are, tools/array.py:91-138 through array.py:1921-1928), N[side] per replicate.
// A side without indices is copied as it is.  With `stats` (xmca_bootstrap_patterns: unrotated, n_out = stats->k) every replicate
// back-projects its k leading modes and queues the pattern kernels behind its solve; lane j owns the accumulators j.
template <typename TI>
void bootstrap_runs_impl(xmca_handle* h, const ComplexOp* op, int axis, const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs,
                         int rotated, int p, int power, double tol, double* spectra, int* kept, int64_t n_out,
                         const PatternStats* stats = nullptr) {
  const int64_t T = h->boot_T;
  const int64_t Nl = h->boot_N[0], Nr = h->boot_fields == 2 ? h->boot_N[1] : 0;
  const int64_t* idx_host[2] = {idx_left, idx_right};
  const int64_t idx_len[2] = {axis == 0 ? T : Nl, axis == 0 ? T : Nr}, bound = axis == 0 ? T : Nl + Nr;
  for (int s = 0; s < 2; ++s)
    if (idx_host[s])
      for (int64_t i = 0; i < n_runs * idx_len[s]; ++i)
        XMCA_CHECK(idx_host[s][i] >= 0 && idx_host[s][i] < bound, XMCA_ERR_INVALID,
                   axis == 0 ? "bootstrap: row index out of range" : "bootstrap: column index out of range");
  const ReplicateSpec spec{T, Nl, Nr, h->boot_fields, op, rotated, p, power, tol, stats ? stats->k : 0};
  const DevBuf<TI>* work = typed<TI>(h).boot;
  run_replicates(h, spec, n_runs, [&](xmca_handle* lh, int64_t first, int64_t stride) {
    DevBuf<int64_t> idx_dev[2];
    DevBuf<double> part, u;      // scratch of the lane's pattern kernels, reused in stream order
    std::function<void(int64_t, const SolveResult&)> after;
    if (stats) {
      XMCA_CHECK(first < stats->lanes, XMCA_ERR_STATE, "bootstrap_patterns: more lanes than accumulators");
      part.ensure((size_t)2 * stats->k * stats->total_tiles);
      u.ensure((size_t)2 * stats->k);
      after = [&, first](int64_t run, const SolveResult& r) { stats->queue_result(lh->st, (int)first, run, r, part.get(), u.get()); };
    }
    // (synchronised after every replicate: the index buffers are overwritten by the next replicate's upload)
    replicate_lane<TI>(lh, "bootstrap", "resample", spec, first, stride, n_runs, true, spectra, kept, n_out, [&](int s, TI* x, int64_t run) {
      const int64_t N = h->boot_N[s];
      const size_t n = (size_t)T * N;
      if (!idx_host[s]) {
        XMCA_HIP(hipMemcpyAsync(x, work[s].get(), sizeof(TI) * n, hipMemcpyDeviceToDevice, lh->st));
        return;
      }
      const int64_t len = idx_len[s];
      XMCA_HIP(hipMemcpyAsync(idx_dev[s].ensure((size_t)len), idx_host[s] + run * len, sizeof(int64_t) * len, hipMemcpyHostToDevice, lh->st));
      if (axis == 0)
        hipLaunchKernelGGL((gather_rows_kernel<TI>), ew_grid((int64_t)n, 4), dim3(EW_BLOCK), 0, lh->st, work[s].get(), x, idx_dev[s].get(),
                           (int)T, N);
      else
        hipLaunchKernelGGL((gather_concat_columns_kernel<TI>), gather_cols_grid(T, N), dim3(GATHER_COLS_BLOCK), 0, lh->st, work[0].get(), Nl,
                           Nr > 0 ? work[1].get() : (const TI*)nullptr, Nr, idx_dev[s].get(), x, N, (int)T);
    }, after);
  });
}

// xmca_bootstrap_runs / xmca_bootstrap_runs_columns (axis 0 / 1): replicates complexified with the Hilbert transform, or real
void bootstrap_runs_entry(xmca_handle* h, int axis, const double* hilbert_col, const int64_t* idx_left, const int64_t* idx_right,
                          int64_t n_runs, int rotated, int p, int power, double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  check_bootstrap_runs(spectra_out, kept_out, n_out, n_runs, rotated, p, power);
  XMCA_CHECK(h->boot_fields >= 1 && h->boot_T > 0, XMCA_ERR_STATE, "bootstrap: call xmca_bootstrap_begin first");
  ComplexOp hop;
  if (hilbert_col) hop = ComplexOp::circulant(hilbert_col, h->boot_T);
  with_dtype(h->dtype, [&](auto t) {
    bootstrap_runs_impl<decltype(t)>(h, hilbert_col ? &hop : nullptr, axis, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out,
                                     kept_out, n_out);
  });
  h->tm.collect();
}

// xmca_bootstrap_runs_extended / xmca_bootstrap_runs_columns_extended: replicates complexified with the extended operator
void bootstrap_runs_extended_entry(xmca_handle* h, int axis, const double* col3, const double* hbar, const double* U, const double* W,
                                   int rank, const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p,
                                   int power, double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  check_bootstrap_runs(spectra_out, kept_out, n_out, n_runs, rotated, p, power);
  check_extended_parts("bootstrap", col3, hbar, U, W, rank);
  XMCA_CHECK(h->boot_fields >= 1 && h->boot_T > 0, XMCA_ERR_STATE, "bootstrap: call xmca_bootstrap_begin first");
  XMCA_CHECK(h->dtype == XMCA_F64, XMCA_ERR_INVALID, "bootstrap: the extended operator needs float64 fields (the reference's replicates are float64)");
  check_operator_size("bootstrap", h->boot_T);
  const ComplexOp op = ComplexOp::extended(col3, hbar, U, W, rank, h->boot_T);
  bootstrap_runs_impl<double>(h, &op, axis, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out, kept_out, n_out);
  h->tm.collect();
}

// xmca_bootstrap_runs_theta / xmca_bootstrap_runs_columns_theta: replicates complexified with the Theta fore/back-cast, every
// replicate fitted again on its lane (ReplicateRunner)
void bootstrap_runs_theta_entry(xmca_handle* h, int axis, const double* col3, const double* hbar, const double* B, int period,
                                const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p, int power,
                                double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  check_bootstrap_runs(spectra_out, kept_out, n_out, n_runs, rotated, p, power);
  XMCA_CHECK(col3 && hbar && B, XMCA_ERR_INVALID, "bootstrap: need col3, hbar and the T x 2 (2 + period) matrix B");
  XMCA_CHECK(h->boot_fields >= 1 && h->boot_T > 0, XMCA_ERR_STATE, "bootstrap: call xmca_bootstrap_begin first");
  XMCA_CHECK(h->dtype == XMCA_F64, XMCA_ERR_INVALID, "bootstrap: the Theta extension needs float64 fields (the reference's replicates are float64)");
  XMCA_CHECK(period >= 1 && h->boot_T >= 2 * (int64_t)period, XMCA_ERR_INVALID, "bootstrap: period must be >= 1 and T >= 2 period");
  check_operator_size("bootstrap", h->boot_T);
  const ComplexOp op = ComplexOp::theta(col3, hbar, B, period, h->boot_T);
  bootstrap_runs_impl<double>(h, &op, axis, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out, kept_out, n_out);
  h->tm.collect();
}

// xmca_bootstrap_patterns: pairs bootstrap of the rows (one index per run, shared by the sides), k vectors per replicate, statistics
void bootstrap_patterns_entry(xmca_handle* h, const double* hilbert_col, const int64_t* idx, int64_t n_runs, int k,
                              const double* const v0_re[2], const double* const v0_im[2], double* const mean_out[2],
                              double* const std_out[2], double* congruence_out, double* sigma_out, int* kept_out) {
  XMCA_CHECK(h->boot_fields >= 1 && h->boot_T > 0, XMCA_ERR_STATE, "bootstrap_patterns: call xmca_bootstrap_begin first");
  const int n_sides = h->boot_fields;
  const bool cplx = hilbert_col != nullptr;
  const int64_t T = h->boot_T;
  XMCA_CHECK(n_runs >= 2, XMCA_ERR_INVALID, "bootstrap_patterns: a standard error needs n_runs >= 2");
  XMCA_CHECK(idx && congruence_out && sigma_out && kept_out, XMCA_ERR_INVALID, "bootstrap_patterns: indices or output buffers missing");
  PatternStats ps;
  ps.n_sides = n_sides;
  ps.cplx = cplx;
  ps.n_runs = n_runs;
  int64_t rank = T;
  for (int s = 0; s < n_sides; ++s) {
    ps.N[s] = h->boot_N[s];
    rank = std::min(rank, ps.N[s]);
    XMCA_CHECK(v0_re[s] && (!cplx || v0_im[s]) && mean_out[s] && std_out[s], XMCA_ERR_INVALID,
               "bootstrap_patterns: the model's vectors or an output is missing for a side");
  }
  XMCA_CHECK(k >= 1 && k <= rank, XMCA_ERR_INVALID, "bootstrap_patterns: k must be between 1 and the rank min(T, N)");
  for (int64_t i = 0; i < n_runs * T; ++i)
    XMCA_CHECK(idx[i] >= 0 && idx[i] < T, XMCA_ERR_INVALID, "bootstrap_patterns: row index out of range");
  ps.k = k;
  const ReplicateSpec shape{T, ps.N[0], n_sides == 2 ? ps.N[1] : 0, n_sides};
  ps.lanes = lanes_for(shape.eig_n(), n_runs);
  ComplexOp hop;
  if (cplx) hop = ComplexOp::circulant(hilbert_col, T);
  ps.begin(h, v0_re, v0_im);
  with_dtype(h->dtype, [&](auto t) {
    bootstrap_runs_impl<decltype(t)>(h, cplx ? &hop : nullptr, 0, idx, n_sides == 2 ? idx : nullptr, n_runs, 0, 0, 1, 0.0, sigma_out,
                                     kept_out, k, &ps);
  });
  ps.finish(h, mean_out, std_out, congruence_out);
  h->tm.collect();
}

// xmca_pattern_stats: host vectors (n_runs x k x N per side and plane) through the kernels of xmca_bootstrap_patterns, run r
// into the accumulators r % n_lanes, all on the handle's stream
template <typename TV>
void pattern_stats_impl(xmca_handle* h, PatternStats& ps, const double* const v0_re[2], const double* const v0_im[2],
                        const double* const v_re[2], const double* const v_im[2], double* const mean_out[2], double* const std_out[2],
                        double* congruence_out) {
  ps.begin(h, v0_re, v0_im);
  DevBuf<double> wide[2][2], part, u;
  Narrow<TV> planes[2];
  const TV* re[2] = {nullptr, nullptr};
  const TV* im[2] = {nullptr, nullptr};
  for (int s = 0; s < ps.n_sides; ++s) {
    const size_t n = (size_t)ps.n_runs * ps.kN(s);
    XMCA_HIP(hipMemcpyAsync(wide[s][0].ensure(n), v_re[s], sizeof(double) * n, hipMemcpyHostToDevice, h->st));
    if (ps.cplx) XMCA_HIP(hipMemcpyAsync(wide[s][1].ensure(n), v_im[s], sizeof(double) * n, hipMemcpyHostToDevice, h->st));
    planes[s].from(h->st, wide[s][0].get(), ps.cplx ? wide[s][1].get() : nullptr, (int64_t)n);
    re[s] = planes[s].r;
    im[s] = planes[s].i;
  }
  part.ensure((size_t)2 * ps.k * ps.total_tiles);
  u.ensure((size_t)2 * ps.k);
  for (int64_t r = 0; r < ps.n_runs; ++r) {
    const TV* rr[2] = {re[0] + r * ps.kN(0), ps.n_sides == 2 ? re[1] + r * ps.kN(1) : nullptr};
    const TV* ri[2] = {ps.cplx ? im[0] + r * ps.kN(0) : nullptr, ps.cplx && ps.n_sides == 2 ? im[1] + r * ps.kN(1) : nullptr};
    ps.queue<TV>(h->st, (int)(r % ps.lanes), r, rr, ri, ps.N, part.get(), u.get());
  }
  ps.finish(h, mean_out, std_out, congruence_out);
}

}  // namespace

template <typename TI>
static void bench_gemm_impl(xmca_handle* h, int M, int N, int K, int a_kfast, int b_nfast, int upper_only, int splits, int reps,
                            double* avg_ms) {
  const int64_t lda = a_kfast ? K : M, ldb = b_nfast ? N : K;
  const size_t na = (size_t)(a_kfast ? M : K) * lda, nb = (size_t)(b_nfast ? K : N) * ldb;
  DevBuf<TI> A, B;
  DevBuf<double> C;
  hipLaunchKernelGGL((philox_normal_kernel<TI>), ew_grid((int64_t)(na + 1) / 2), dim3(EW_BLOCK), 0, h->st, A.ensure(na), (int64_t)na,
                     (uint64_t)1, 0u, 0u);
  hipLaunchKernelGGL((philox_normal_kernel<TI>), ew_grid((int64_t)(nb + 1) / 2), dim3(EW_BLOCK), 0, h->st, B.ensure(nb), (int64_t)nb,
                     (uint64_t)2, 0u, 1u);
  C.ensure((size_t)M * N);
  GemmOpts o;
  o.a_kfast = a_kfast != 0; o.b_nfast = b_nfast != 0; o.upper_only = upper_only != 0; o.mirror = upper_only ? 1 : 0;
  o.force_splits = splits;
  hipEvent_t e0, e1;
  XMCA_HIP(hipEventCreate(&e0));
  XMCA_HIP(hipEventCreate(&e1));
  gemm<TI, double>(h->st, h->gws, A.get(), lda, B.get(), ldb, C.get(), N, M, N, K, o);
  XMCA_HIP(hipStreamSynchronize(h->st));
  XMCA_HIP(hipEventRecord(e0, h->st));
  for (int i = 0; i < reps; ++i) gemm<TI, double>(h->st, h->gws, A.get(), lda, B.get(), ldb, C.get(), N, M, N, K, o);
  XMCA_HIP(hipEventRecord(e1, h->st));
  XMCA_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  XMCA_HIP(hipEventElapsedTime(&ms, e0, e1));
  *avg_ms = ms / reps;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}


extern "C" {

// checks and state changes shared by xmca_set_field and xmca_set_field_strided: left before right, one dtype, one T
static void begin_set_field(xmca_handle* h, int side, const void* re, int64_t T, int64_t N, int dtype) {
  check_side("set_field", side);
  XMCA_CHECK(re && T >= 2 && N >= 1, XMCA_ERR_INVALID, "set_field: need a T x N field with T >= 2, N >= 1");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, "set_field: dtype must be float32 or float64");
  XMCA_CHECK(T < (1 << 30) && N < (1ll << 31), XMCA_ERR_UNSUPPORTED, "set_field: dimension too large");
  if (side == 0) { h->field_set[1] = false; h->dtype = dtype; }
  else {
    XMCA_CHECK(h->field_set[0], XMCA_ERR_STATE, "set_field: set the left field first");
    XMCA_CHECK(dtype == h->dtype, XMCA_ERR_INVALID, "set_field: both fields must have the same dtype");
    XMCA_CHECK(T == resident_T(h), XMCA_ERR_INVALID, "set_field: time dimensions of the fields differ");
  }
}
static void end_set_field(xmca_handle* h, int side) {
  h->field_set[side] = true;
  h->solved = false;
  if (side == 0) h->op_pending = false;
}

int xmca_set_field(xmca_handle* h, int side, const void* re, const void* im, int64_t T, int64_t N, int dtype, int location) {
  API_BEGIN(h)
  begin_set_field(h, side, re, T, N, dtype);
  with_dtype(dtype, [&](auto t) { set_field_impl<decltype(t)>(h, side, re, im, T, N, location); });
  end_set_field(h, side);
  API_END(h)
}

int xmca_ingest_regime(int64_t T, int64_t N, int64_t stride_t, int64_t stride_n) {
  if (T < 1 || N < 1 || stride_t < 0 || stride_n < 0) return XMCA_ERR_INVALID;
  return ingest_regime(T, N, stride_t, stride_n);
}

int xmca_set_field_strided(xmca_handle* h, int side, const void* re, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype) {
  API_BEGIN(h)
  begin_set_field(h, side, re, T, N, dtype);
  XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, "set_field_strided: strides must not be negative");
  check_device_pointer(h, "set_field_strided", re);
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    FieldData<TI>& f = typed<TI>(h).f[side];
    f.T = T; f.N = N;
    f.has_im = false;
    f.ext_re = nullptr; f.ext_im = nullptr;
    h->tm.begin("ingest_strided");
    ingest_strided<TI>(h->st, static_cast<const TI*>(re), T, N, stride_t, stride_n, f.re.ensure((size_t)T * N));
    XMCA_HIP(hipGetLastError());
    h->tm.end();
    XMCA_HIP(hipStreamSynchronize(h->st));        // (the caller's memory is not referenced after the call)
  });
  end_set_field(h, side);
  API_END(h)
}

int xmca_complexify(xmca_handle* h, const double* hilbert_col) {
  API_BEGIN(h)
  XMCA_CHECK(h->field_set[0], XMCA_ERR_STATE, "complexify: set a field first");
  if (!hilbert_col) {            // back to the real fields (their real planes are untouched by a complex solve)
    h->op_pending = false;
    for (int s = 0; s < 2; ++s) { h->s32.f[s].has_im = false; h->s64.f[s].has_im = false; }      // (both dtypes' fields)
    h->solved = false;
    return XMCA_OK;
  }
  h->op = ComplexOp::circulant(hilbert_col, resident_T(h));
  h->op_pending = true;           // xmca_solve decides: subspace formulation (no imaginary plane) or X_im = Ht X
  h->solved = false;
  API_END(h)
}

// the resident real float32 fields become float64 fields (xmca_complexify_extended, xmca_complexify_theta)
static void promote_fields(xmca_handle* h) {
  if (h->dtype == XMCA_F32) {     // (not a dispatch: only float32 fields are moved, from typed<float> to typed<double>)
    // the reference extends in float64 (the forecast of a float32 column is float64, array.py:394-410): the resident real
    // float32 fields become float64 fields, exactly (every float32 is a float64)
    for (int s = 0; s < 2; ++s) {
      if (!h->field_set[s]) continue;
      FieldData<float>& a = h->s32.f[s];
      FieldData<double>& b = h->s64.f[s];
      const int64_t n = a.T * a.N;
      b.T = a.T; b.N = a.N; b.has_im = false; b.ext_re = nullptr; b.ext_im = nullptr;
      hipLaunchKernelGGL((convert_kernel<float, double>), ew_grid(n), dim3(EW_BLOCK), 0, h->st, a.r(), b.re.ensure((size_t)n), n);
      XMCA_HIP(hipGetLastError());
    }
    XMCA_HIP(hipStreamSynchronize(h->st));
    for (int s = 0; s < 2; ++s) {
      FieldData<float>& a = h->s32.f[s];
      a.re.release(); a.im.release(); a.ext_re = nullptr; a.ext_im = nullptr; a.has_im = false;
    }
    h->dtype = XMCA_F64;
  }
}

int xmca_complexify_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W, int rank) {
  API_BEGIN(h)
  XMCA_CHECK(h->field_set[0], XMCA_ERR_STATE, "complexify_extended: set a field first");
  check_extended_parts("complexify_extended", col3, hbar, U, W, rank);
  promote_fields(h);
  const int64_t T = h->s64.f[0].T;
  check_operator_size("complexify_extended", T);
  h->op = ComplexOp::extended(col3, hbar, U, W, rank, T);
  h->op_pending = true;           // xmca_solve / xmca_project form X_im = G X (there is no subspace formulation of G)
  h->solved = false;
  API_END(h)
}

int xmca_complexify_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period) {
  API_BEGIN(h)
  XMCA_CHECK(h->field_set[0], XMCA_ERR_STATE, "complexify_theta: set a field first");
  XMCA_CHECK(col3 && hbar && B, XMCA_ERR_INVALID, "complexify_theta: need col3, hbar and the T x 2 (2 + period) matrix B");
  const int64_t T = resident_T(h);
  XMCA_CHECK(period >= 1 && T >= 2 * (int64_t)period, XMCA_ERR_INVALID, "complexify_theta: period must be >= 1 and T >= 2 period");
  check_operator_size("complexify_theta", T);
  promote_fields(h);
  h->op = ComplexOp::theta(col3, hbar, B, period, T);
  h->op_pending = true;           // xmca_solve / xmca_project / xmca_get_field_imag form X_im = G0 X + B C
  h->solved = false;
  API_END(h)
}

int xmca_theta_fit(xmca_handle* h, int side, int period, double* out) {
  API_BEGIN(h)
  check_side("theta_fit", side);
  XMCA_CHECK(h->field_set[side] && out, XMCA_ERR_STATE, "theta_fit: set the field first");
  const int64_t T = resident_T(h), N = resident_N(h, side);
  XMCA_CHECK(period >= 1 && T >= 2 * (int64_t)period, XMCA_ERR_INVALID, "theta_fit: period must be >= 1 and T >= 2 period");
  check_operator_size("theta_fit", T);
  const int64_t rows = theta_fit_rows(period), keep = 3 + period;
  DevBuf<double> wide, fit;
  const double* x = nullptr;
  with_dtype(h->dtype, [&](auto t) {
    using TI = decltype(t);
    const FieldData<TI>& f = typed<TI>(h).f[side];
    if constexpr (std::is_same<TI, double>::value) {
      x = f.r();
    } else {
      hipLaunchKernelGGL((convert_kernel<float, double>), ew_grid(T * N), dim3(EW_BLOCK), 0, h->st, f.r(), wide.ensure((size_t)(T * N)), T * N);
      XMCA_HIP(hipGetLastError());
      x = wide.get();
    }
  });
  theta_fit(h->st, x, T, N, period, fit.ensure((size_t)(2 * rows * N)));
  std::vector<double> host((size_t)(2 * rows * N));
  XMCA_HIP(hipMemcpyAsync(host.data(), fit.get(), sizeof(double) * host.size(), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  for (int d = 0; d < 2; ++d)
    for (int64_t r = 0; r < keep; ++r)       // alpha, b0, level, then the seasonal means (the two forecast coefficients between are left out)
      std::memcpy(out + (d * keep + r) * N, host.data() + (d * rows + (r < 3 ? r : r + 2)) * N, sizeof(double) * (size_t)N);
  API_END(h)
}

int xmca_get_field_imag(xmca_handle* h, int side, double* out) {
  API_BEGIN(h)
  check_side("get_field_imag", side);
  XMCA_CHECK(h->field_set[side] && out, XMCA_ERR_STATE, "get_field_imag: no field resident for this side");
  XMCA_CHECK(h->dtype == XMCA_F64, XMCA_ERR_STATE, "get_field_imag: only after xmca_complexify_extended / xmca_complexify_theta");
  if (h->op_pending && h->op.kind != ComplexOp::CIRCULANT) {
    complexify_impl<double>(h, h->op);
    h->op_pending = false;
  }
  const FieldData<double>& f = h->s64.f[side];
  XMCA_CHECK(f.has_im && f.i(), XMCA_ERR_STATE, "get_field_imag: the field has no imaginary plane");
  XMCA_HIP(hipMemcpyAsync(out, f.i(), sizeof(double) * (size_t)f.T * f.N, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_solve(xmca_handle* h, int n_fields, int64_t n_vec, int64_t* rank_out) {
  API_BEGIN(h)
  XMCA_CHECK(n_fields == 1 || n_fields == 2, XMCA_ERR_INVALID, "solve: n_fields must be 1 or 2");
  XMCA_CHECK(h->field_set[0] && (n_fields == 1 || h->field_set[1]), XMCA_ERR_STATE, "solve: fields not set");
  h->solved = false;
  with_dtype(h->dtype, [&](auto t) { solve_impl<decltype(t)>(h, n_fields, n_vec); });
  if (n_fields == 1) h->res.ldv[1] = 0;      // (a one-field result has no right vectors: xmca_rotate_solved stacks by ldv)
  h->solved = true;
  if (rank_out) *rank_out = h->res.rank;
  h->tm.collect();
  API_END(h)
}

int xmca_get_singular_values(xmca_handle* h, double* out, int64_t n) {
  API_BEGIN_NO_JOIN(h)               // (host values, final when solve returned)
  XMCA_CHECK(h->solved, XMCA_ERR_STATE, "singular values requested before solve");
  XMCA_CHECK(out && n >= 0 && n <= h->res.rank, XMCA_ERR_INVALID, "get_singular_values: bad size");
  std::memcpy(out, h->res.sigma.data(), sizeof(double) * (size_t)n);
  API_END(h)
}

int xmca_is_complex(xmca_handle* h) { return (h && h->solved && h->res.cplx) ? 1 : 0; }

long long xmca_persistent_giveups(void) { return (long long)::xmca::persist_giveups().load(); }

int xmca_vectors_are_f32(xmca_handle* h, int side) {
  return (h && h->solved && (side == 0 || side == 1) && h->res.vt_f32[side]) ? 1 : 0;
}

int xmca_get_solve_info(xmca_handle* h, int* info, int n) {
  if (!h || !info) return XMCA_ERR_INVALID;
  for (int i = 0; i < n && i < 9; ++i) {
    const EvdInfo& e = h->res.evd_info[i / 3];
    info[i] = (i % 3 == 0) ? e.sweeps : (i % 3 == 1) ? e.tile : e.slots;
  }
  for (int i = 9; i < n && i < 12; ++i) info[i] = h->res.evd_info[i - 9].lr_step + 2 * h->res.evd_info[i - 9].tridiag;   // bit 1: tridiagonal route
  for (int i = 12; i < n && i < 15; ++i) info[i] = h->res.evd_info[i - 12].n_eigvec;
  if (n > 15) info[15] = h->solved ? h->res.n_vec : 0;
  for (int i = 16; i < n && i < 18; ++i) {       // KiB of the device blocks that hold the vector planes of side i - 16
    const SolveResult& r = h->res;
    const int s = i - 16;
    const size_t bytes = r.Vt[s].re.cap_bytes + r.Vt[s].im.cap_bytes + r.Vt32[s].cap_bytes;
    info[i] = (int)((bytes + 1023) / 1024);
  }
  return XMCA_OK;
}

int xmca_get_vectors(xmca_handle* h, int side, void* out, int64_t n_modes, int dtype) {
  API_BEGIN_NO_JOIN(h)
  if (n_modes > h->tail.head) join_tail(h);       // (the modes of the head were complete when solve returned)
  XMCA_CHECK(h->solved, XMCA_ERR_STATE, "vectors requested before solve");
  check_side("get_vectors", side);
  XMCA_CHECK(out && n_modes >= 0 && n_modes <= h->res.n_vec && h->res.ldv[side] > 0, XMCA_ERR_INVALID,
             "get_vectors: more modes requested than were back-projected");
  if (n_modes > 0) with_dtype(dtype, [&](auto t) { get_vectors_impl<decltype(t)>(h, side, out, n_modes); });
  API_END(h)
}

int xmca_get_eofs(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, void* out, int dtype) {
  API_BEGIN(h)
  XMCA_CHECK(h->solved, XMCA_ERR_STATE, "eofs requested before solve");
  check_side("get_eofs", side);
  XMCA_CHECK(out && q >= 1 && m >= 1 && m <= h->res.n_vec && (W || q == m) && h->res.ldv[side] > 0, XMCA_ERR_INVALID,
             "get_eofs: more modes requested than were back-projected, or a bad mixing matrix");
  with_dtype(dtype, [&](auto t) { get_eofs_impl<decltype(t)>(h, side, W, m, q, w_is_complex != 0, out); });
  API_END(h)
}

int xmca_get_maps(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, const double* col_factor,
                  int factor_is_complex, const int64_t* keep_idx, int64_t N_full, int kind, int scaling, void* out, int dtype,
                  double* stat_out) {
  return xmca_get_maps_to(h, side, W, m, q, w_is_complex, col_factor, factor_is_complex, keep_idx, N_full, kind, scaling, out, dtype,
                          stat_out, XMCA_HOST);
}

int xmca_get_maps_to(xmca_handle* h, int side, const double* W, int64_t m, int64_t q, int w_is_complex, const double* col_factor,
                     int factor_is_complex, const int64_t* keep_idx, int64_t N_full, int kind, int scaling, void* out, int dtype,
                     double* stat_out, int out_location) {
  API_BEGIN(h)
  XMCA_CHECK(h->solved, XMCA_ERR_STATE, "maps requested before solve");
  check_side("get_maps", side);
  XMCA_CHECK(out && q >= 1 && q <= INT32_MAX && m >= 1 && m <= h->res.n_vec && (W || q == m) && h->res.ldv[side] > 0, XMCA_ERR_INVALID,
             "get_maps: more modes requested than were back-projected, or a bad mixing matrix");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, "get_maps: dtype must be XMCA_F32 or XMCA_F64");
  check_out_location(h, "get_maps", out_location, out);
  XMCA_CHECK((kind == XMCA_MAP_EOF && (scaling == XMCA_SCALE_NONE || scaling == XMCA_SCALE_MAX || scaling == XMCA_SCALE_STD)) ||
                 (kind == XMCA_MAP_AMPLITUDE && (scaling == XMCA_SCALE_NONE || scaling == XMCA_SCALE_MAX)) ||
                 (kind == XMCA_MAP_PHASE && scaling == XMCA_SCALE_NONE),
             XMCA_ERR_INVALID, "get_maps: EOFs scale by NONE / MAX / STD, amplitudes by NONE / MAX, phases not at all");
  check_kept_columns("get_maps", keep_idx, h->res.ldv[side], N_full, INT32_MAX);      // (kept columns: the rows of the vectors)
  with_dtype(dtype, [&](auto t) {
    get_maps_impl<decltype(t)>(h, side, W, m, q, w_is_complex != 0, col_factor, factor_is_complex != 0, keep_idx, N_full, kind, scaling,
                               out, stat_out, out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_project(xmca_handle* h, int side, const void* V, int64_t N, int64_t m, int is_complex, void* U_out,
                 int* out_is_complex) {
  API_BEGIN(h)
  check_side("project", side);
  XMCA_CHECK(h->field_set[side], XMCA_ERR_STATE, "project: no field resident for this side");
  XMCA_CHECK(U_out && out_is_complex && N >= 1 && m >= 1, XMCA_ERR_INVALID, "project: need an N x m matrix of vectors");
  if (!V)
    XMCA_CHECK(h->solved && m <= h->res.n_vec && h->res.ldv[side] == N, XMCA_ERR_INVALID,
               "project: the resident vectors of the last solve do not have N rows and m modes");
  with_dtype(h->dtype, [&](auto t) { project_impl<decltype(t)>(h, side, V, N, m, is_complex != 0, U_out, out_is_complex); });
  API_END(h)
}

int xmca_predict(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int dtype, const int64_t* keep_idx,
                 int64_t N_keep, const void* mean, const void* std, const void* V, int v_is_complex, const double* W, int64_t m,
                 int64_t q, int w_is_complex, double* out, int* out_is_complex) {
  return xmca_predict_weighted(h, side, X, T_new, N_full, dtype, keep_idx, N_keep, mean, std, V, v_is_complex, W, m, q, w_is_complex, out,
                               out_is_complex, nullptr);
}

int xmca_predict_weighted(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int dtype, const int64_t* keep_idx,
                          int64_t N_keep, const void* mean, const void* std, const void* V, int v_is_complex, const double* W, int64_t m,
                          int64_t q, int w_is_complex, double* out, int* out_is_complex, const double* weight) {
  return xmca_predict_strided(h, side, X, T_new, N_full, N_full, 1, XMCA_HOST, dtype, keep_idx, N_keep, mean, std, V, v_is_complex, W, m, q,
                              w_is_complex, out, out_is_complex, weight);
}

int xmca_predict_strided(xmca_handle* h, int side, const void* X, int64_t T_new, int64_t N_full, int64_t stride_t, int64_t stride_n,
                         int x_location, int dtype, const int64_t* keep_idx, int64_t N_keep, const void* mean, const void* std,
                         const void* V, int v_is_complex, const double* W, int64_t m, int64_t q, int w_is_complex, double* out,
                         int* out_is_complex, const double* weight) {
  API_BEGIN(h)
  check_transform(h, "predict", side, V, m, keep_idx, N_keep, N_full);
  XMCA_CHECK(X && mean && W && out && out_is_complex && T_new >= 1 && m >= 1 && q >= 1 && q <= INT32_MAX, XMCA_ERR_INVALID,
             "predict: need new data, means, an m x q mix (m, q >= 1) and an output");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, "predict: dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(x_location == XMCA_HOST || x_location == XMCA_DEVICE, XMCA_ERR_INVALID, "predict: the location must be XMCA_HOST or XMCA_DEVICE");
  if (x_location == XMCA_DEVICE) {
    XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, "predict: strides must not be negative");
    check_device_pointer(h, "predict", X);
  } else {
    XMCA_CHECK(stride_t == N_full && stride_n == 1, XMCA_ERR_INVALID, "predict: host data must be contiguous rows");
  }
  const bool vt32 = !V && h->res.vt_f32[side];
  const bool vc = v_is_complex != 0, wc = w_is_complex != 0;
  // 2 x 2: the data's element type TI (the ingest arithmetic) x the resident vectors' element type TP (the product)
  with_dtype(dtype, [&](auto ti) {
    using TI = decltype(ti);
    with_dtype(vt32 ? XMCA_F32 : XMCA_F64, [&](auto tp) {
      predict_impl<TI, decltype(tp)>(h, side, static_cast<const TI*>(X), x_location == XMCA_DEVICE, stride_t, stride_n, T_new, N_full,
                                     keep_idx, N_keep, static_cast<const TI*>(mean),
                                     static_cast<const TI*>(std), weight, V, vc, W, m, q, wc, out, out_is_complex);
    });
  });
  API_END(h)
}

int xmca_reconstruct(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V, int v_is_complex,
                     const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean, const double* std, double* out) {
  return xmca_reconstruct_weighted(h, side, B, T, m, b_is_complex, V, v_is_complex, keep_idx, N_keep, N_full, mean, std, out, nullptr);
}

int xmca_reconstruct_weighted(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V,
                              int v_is_complex, const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean,
                              const double* std, double* out, const double* inv_weight) {
  return xmca_reconstruct_to(h, side, B, T, m, b_is_complex, V, v_is_complex, keep_idx, N_keep, N_full, mean, std, out, inv_weight,
                             XMCA_HOST);
}

int xmca_reconstruct_to(xmca_handle* h, int side, const double* B, int64_t T, int64_t m, int b_is_complex, const void* V,
                        int v_is_complex, const int64_t* keep_idx, int64_t N_keep, int64_t N_full, const double* mean,
                        const double* std, double* out, const double* inv_weight, int out_location) {
  API_BEGIN(h)
  check_transform(h, "reconstruct", side, V, m, keep_idx, N_keep, N_full);
  XMCA_CHECK(out && T >= 1 && (B || m == 0), XMCA_ERR_INVALID, "reconstruct: need a T x m coefficient matrix and an output");
  check_out_location(h, "reconstruct", out_location, out);
  // the product runs in the element type of the resident vectors it reads (float64 for host vectors)
  with_dtype(m > 0 && !V && h->res.vt_f32[side] ? XMCA_F32 : XMCA_F64, [&](auto tp) {
    reconstruct_impl<decltype(tp)>(h, side, B, T, m, b_is_complex != 0, V, v_is_complex != 0, keep_idx, N_keep, N_full, mean, std, inv_weight,
                                   out, out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_center_field(xmca_handle* h, int side, double* mean_out, double* std_out, int64_t* n_nan_out) {
  API_BEGIN(h)
  check_side("center_field", side);
  XMCA_CHECK(h->field_set[side] && mean_out && std_out && n_nan_out, XMCA_ERR_STATE, "center_field: set the field first");
  with_dtype(h->dtype, [&](auto t) { center_field_impl<decltype(t)>(h, side, mean_out, std_out, n_nan_out); });
  API_END(h)
}

int xmca_compact_field(xmca_handle* h, int side, int* keep_out, int64_t* n_keep_out) {
  API_BEGIN(h)
  check_side("compact_field", side);
  XMCA_CHECK(h->field_set[side] && keep_out && n_keep_out, XMCA_ERR_STATE, "compact_field: set the field first");
  with_dtype(h->dtype, [&](auto t) { compact_field_impl<decltype(t)>(h, side, keep_out, n_keep_out); });
  h->solved = false;
  API_END(h)
}

int xmca_scale_field(xmca_handle* h, int side, const void* w, int divide) {
  API_BEGIN(h)
  check_side("scale_field", side);
  XMCA_CHECK(h->field_set[side] && w, XMCA_ERR_STATE, "scale_field: set the field first");
  with_dtype(h->dtype, [&](auto t) { scale_field_impl<decltype(t)>(h, side, w, divide); });
  h->solved = false;
  API_END(h)
}

int xmca_get_field(xmca_handle* h, int side, void* out) {
  API_BEGIN(h)
  XMCA_CHECK((side == 0 || side == 1) && out, XMCA_ERR_INVALID, "get_field: bad arguments");
  XMCA_CHECK(h->field_set[side], XMCA_ERR_STATE, "get_field: no field resident for this side");
  with_dtype(h->dtype, [&](auto t) {
    using TI = decltype(t);
    const FieldData<TI>& f = typed<TI>(h).f[side];
    XMCA_HIP(hipMemcpyAsync(out, f.r(), sizeof(TI) * (size_t)f.T * f.N, hipMemcpyDeviceToHost, h->st));
  });
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_bootstrap_begin(xmca_handle* h, int n_fields) {
  API_BEGIN(h)
  XMCA_CHECK(n_fields == 1 || n_fields == 2, XMCA_ERR_INVALID, "bootstrap: n_fields must be 1 or 2");
  with_dtype(h->dtype, [&](auto t) { bootstrap_begin_impl<decltype(t)>(h, n_fields); });
  API_END(h)
}

int xmca_bootstrap_runs(xmca_handle* h, const double* hilbert_col, const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs,
                        int rotated, int p, int power, double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_entry(h, 0, hilbert_col, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out, kept_out, n_out);
  API_END(h)
}

int xmca_bootstrap_runs_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W, int rank,
                                 const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p, int power,
                                 double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_extended_entry(h, 0, col3, hbar, U, W, rank, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out, kept_out,
                                n_out);
  API_END(h)
}

int xmca_bootstrap_runs_columns(xmca_handle* h, const double* hilbert_col, const int64_t* cols_left, const int64_t* cols_right,
                                int64_t n_runs, int rotated, int p, int power, double tol, double* spectra_out, int* kept_out,
                                int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_entry(h, 1, hilbert_col, cols_left, cols_right, n_runs, rotated, p, power, tol, spectra_out, kept_out, n_out);
  API_END(h)
}

int xmca_bootstrap_runs_columns_extended(xmca_handle* h, const double* col3, const double* hbar, const double* U, const double* W,
                                         int rank, const int64_t* cols_left, const int64_t* cols_right, int64_t n_runs, int rotated,
                                         int p, int power, double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_extended_entry(h, 1, col3, hbar, U, W, rank, cols_left, cols_right, n_runs, rotated, p, power, tol, spectra_out,
                                kept_out, n_out);
  API_END(h)
}

int xmca_bootstrap_runs_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period,
                              const int64_t* idx_left, const int64_t* idx_right, int64_t n_runs, int rotated, int p, int power,
                              double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_theta_entry(h, 0, col3, hbar, B, period, idx_left, idx_right, n_runs, rotated, p, power, tol, spectra_out, kept_out,
                             n_out);
  API_END(h)
}

int xmca_bootstrap_runs_columns_theta(xmca_handle* h, const double* col3, const double* hbar, const double* B, int period,
                                      const int64_t* cols_left, const int64_t* cols_right, int64_t n_runs, int rotated, int p,
                                      int power, double tol, double* spectra_out, int* kept_out, int64_t n_out) {
  API_BEGIN(h)
  bootstrap_runs_theta_entry(h, 1, col3, hbar, B, period, cols_left, cols_right, n_runs, rotated, p, power, tol, spectra_out, kept_out,
                             n_out);
  API_END(h)
}

int xmca_bootstrap_patterns(xmca_handle* h, const double* hilbert_col, const int64_t* idx, int64_t n_runs, int k,
                            const double* v0_left_re, const double* v0_left_im, const double* v0_right_re, const double* v0_right_im,
                            double* mean_left, double* std_left, double* mean_right, double* std_right, double* congruence_out,
                            double* sigma_out, int* kept_out) {
  API_BEGIN(h)
  const double* const v0_re[2] = {v0_left_re, v0_right_re};
  const double* const v0_im[2] = {v0_left_im, v0_right_im};
  double* const mean_out[2] = {mean_left, mean_right};
  double* const std_out[2] = {std_left, std_right};
  bootstrap_patterns_entry(h, hilbert_col, idx, n_runs, k, v0_re, v0_im, mean_out, std_out, congruence_out, sigma_out, kept_out);
  API_END(h)
}

int xmca_pattern_stats(xmca_handle* h, const double* v0_left_re, const double* v0_left_im, const double* v0_right_re,
                       const double* v0_right_im, const double* v_left_re, const double* v_left_im, const double* v_right_re,
                       const double* v_right_im, int64_t n_runs, int k, int64_t N_left, int64_t N_right, int is_complex, int plane_dtype,
                       int n_lanes, double* mean_left, double* std_left, double* mean_right, double* std_right,
                       double* congruence_out) {
  API_BEGIN(h)
  const bool cplx = is_complex != 0;
  const double* const v0_re[2] = {v0_left_re, v0_right_re};
  const double* const v0_im[2] = {v0_left_im, v0_right_im};
  const double* const v_re[2] = {v_left_re, v_right_re};
  const double* const v_im[2] = {v_left_im, v_right_im};
  double* const mean_out[2] = {mean_left, mean_right};
  double* const std_out[2] = {std_left, std_right};
  XMCA_CHECK(n_runs >= 2 && n_runs <= (1 << 20) && k >= 1 && k <= 65535 && N_left >= 1 && N_right >= 0 && n_lanes >= 1 && n_lanes <= 8 &&
                 congruence_out,
             XMCA_ERR_INVALID, "pattern_stats: need n_runs >= 2, 1 <= k <= 65535, N_left >= 1 and 1 <= n_lanes <= 8");
  XMCA_CHECK(plane_dtype == XMCA_F32 || plane_dtype == XMCA_F64, XMCA_ERR_INVALID, "pattern_stats: plane_dtype must be XMCA_F32 or XMCA_F64");
  PatternStats ps;
  ps.k = k;
  ps.n_sides = N_right > 0 ? 2 : 1;
  ps.lanes = n_lanes;
  ps.cplx = cplx;
  ps.n_runs = n_runs;
  ps.N[0] = N_left;
  ps.N[1] = N_right;
  for (int s = 0; s < ps.n_sides; ++s)
    XMCA_CHECK(v0_re[s] && v_re[s] && (!cplx || (v0_im[s] && v_im[s])) && mean_out[s] && std_out[s], XMCA_ERR_INVALID,
               "pattern_stats: vectors or an output missing for a side");
  with_dtype(plane_dtype, [&](auto tv) {
    pattern_stats_impl<decltype(tv)>(h, ps, v0_re, v0_im, v_re, v_im, mean_out, std_out, congruence_out);
  });
  API_END(h)
}

int xmca_pattern_tile(void) { return PATTERN_TILE; }

int xmca_lag_gram_tile(void) { return LAG_TILE; }

int xmca_lag_gram(xmca_handle* h, const double* G, int64_t n, int embedding, int tau, int center, double* K_out) {
  API_BEGIN(h)
  XMCA_CHECK(G && K_out && n >= 1 && embedding >= 1 && tau >= 1, XMCA_ERR_INVALID, "lag_gram: bad arguments");
  check_operator_size("lag_gram", n);
  const int64_t np = n - (int64_t)(embedding - 1) * tau;
  XMCA_CHECK(np >= 1, XMCA_ERR_INVALID, "lag_gram: (embedding - 1) * tau must be below n");
  DevBuf<double> Gd, K, part, mean;
  XMCA_HIP(hipMemcpyAsync(Gd.ensure((size_t)n * n), G, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, h->st));
  h->tm.begin("lag_gram");
  lag_gram(h->st, Gd.get(), n, (int)n, embedding, tau, center != 0, K.ensure((size_t)np * np), part, mean);
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(K_out, K.get(), sizeof(double) * (size_t)np * np, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_extended_eofs(xmca_handle* h, int embedding, int tau, int n_modes, const int64_t* keep_idx, int64_t N_full, double* lam_out,
                       double* pcs_out, double* eofs_out) {
  API_BEGIN(h)
  // (the outputs and n_modes come before the embedding wherever a field is set, as ever: with a T above the operator's bound a
  // missing output is INVALID, not UNSUPPORTED)
  XMCA_CHECK(!h->field_set[0] || (lam_out && pcs_out && eofs_out && n_modes >= 1), XMCA_ERR_INVALID, "extended_eofs: bad arguments");
  const int64_t np = check_lag_embedding(h, "extended_eofs", embedding, tau, 2);
  const int64_t N = resident_N(h, 0);
  XMCA_CHECK(n_modes <= np - 1 && n_modes <= (int64_t)embedding * N, XMCA_ERR_INVALID,
             "extended_eofs: n_modes must not exceed min(T' - 1, embedding * N)");
  XMCA_CHECK(N < ((int64_t)1 << 31) && (int64_t)embedding * n_modes * std::max(N, N_full) < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED,
             "extended_eofs: pattern array too large");
  // (no INT32_MAX bound on N_full here: this entry's size limits are the two above, which the assembly kernels index within)
  check_kept_columns("extended_eofs", keep_idx, N, N_full, INT64_MAX);
  with_dtype(h->dtype, [&](auto t) {
    extended_eofs_impl<decltype(t)>(h, embedding, tau, n_modes, keep_idx, N_full, lam_out, pcs_out, eofs_out);
  });
  API_END(h)
}

int xmca_gap_fill_tile(int* rows_out, int* cols_out) {
  if (!rows_out || !cols_out) return XMCA_ERR_INVALID;
  *rows_out = GAP_ROWS;
  *cols_out = GAP_COLS;
  return XMCA_OK;
}

// The checks and the call shared by xmca_fill_gaps (embedding = tau = 1) and xmca_fill_gaps_lagged
static void fill_gaps_entry(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, const int64_t* cv_idx, int64_t n_cv, int n_modes,
                            int embedding, int tau, int max_iter, double tol, void* out, double* history_out, int* iters_out,
                            double* cv_rms_out, double* lam_out) {
  XMCA_CHECK(X && out && history_out && iters_out && cv_rms_out && lam_out && n_cv >= 0 && (cv_idx || n_cv == 0), XMCA_ERR_INVALID,
             "fill_gaps: bad arguments");
  check_gap_plane("fill_gaps", T, N, dtype);
  XMCA_CHECK(embedding >= 1 && tau >= 1, XMCA_ERR_INVALID, "fill_gaps: embedding and tau must be at least 1");
  const int64_t np = T - (int64_t)(embedding - 1) * tau;
  if (embedding == 1) {
    XMCA_CHECK(n_modes >= 1 && n_modes <= std::min(T, N) - 1, XMCA_ERR_INVALID, "fill_gaps: n_modes must lie in [1, min(T, N) - 1]");
  } else {
    XMCA_CHECK(np >= 2, XMCA_ERR_INVALID, "fill_gaps: T - (embedding - 1) * tau must be at least 2");
    XMCA_CHECK(tau <= np, XMCA_ERR_INVALID, "fill_gaps: tau above T' leaves time steps outside every window (no reconstruction there)");
    XMCA_CHECK(n_modes >= 1 && n_modes <= std::min<int64_t>(np, (int64_t)embedding * N) - 1, XMCA_ERR_INVALID,
               "fill_gaps: n_modes must lie in [1, min(T', embedding * N) - 1]");
    XMCA_CHECK((int64_t)embedding * n_modes * N < ((int64_t)1 << 34), XMCA_ERR_UNSUPPORTED, "fill_gaps: coefficient matrices too large");
  }
  XMCA_CHECK(max_iter >= 1, XMCA_ERR_INVALID, "fill_gaps: max_iter must be at least 1");
  XMCA_CHECK(std::isfinite(tol) && tol >= 0.0, XMCA_ERR_INVALID, "fill_gaps: tol must be finite and not negative");
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    const TI* Xt = static_cast<const TI*>(X);
    const int64_t n_present = gap_check_field<TI>("fill_gaps", Xt, T, N);
    gap_check_withheld<TI>(Xt, T * N, cv_idx, n_cv);
    fill_gaps_impl<TI>(h, Xt, (int)T, N, n_present, cv_idx, n_cv, n_modes, embedding, embedding == 1 ? 1 : tau, max_iter, tol,
                       static_cast<TI*>(out), history_out, iters_out, cv_rms_out, lam_out);
  });
}

int xmca_fill_gaps(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, const int64_t* cv_idx, int64_t n_cv, int n_modes,
                   int max_iter, double tol, void* out, double* history_out, int* iters_out, double* cv_rms_out, double* lam_out) {
  API_BEGIN(h)
  fill_gaps_entry(h, X, T, N, dtype, cv_idx, n_cv, n_modes, 1, 1, max_iter, tol, out, history_out, iters_out, cv_rms_out, lam_out);
  API_END(h)
}

int xmca_fill_gaps_lagged(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, const int64_t* cv_idx, int64_t n_cv, int n_modes,
                          int embedding, int tau, int max_iter, double tol, void* out, double* history_out, int* iters_out,
                          double* cv_rms_out, double* lam_out) {
  API_BEGIN(h)
  fill_gaps_entry(h, X, T, N, dtype, cv_idx, n_cv, n_modes, embedding, tau, max_iter, tol, out, history_out, iters_out, cv_rms_out, lam_out);
  API_END(h)
}

int xmca_gap_center(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, double* mean_out, unsigned char* mask_out, double* A_out,
                    double* scale_out) {
  API_BEGIN(h)
  XMCA_CHECK(X && mean_out && mask_out && A_out && scale_out, XMCA_ERR_INVALID, "gap_center: bad arguments");
  check_gap_plane("gap_center", T, N, dtype);
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    gap_check_field<TI>("gap_center", static_cast<const TI*>(X), T, N);
    gap_center_impl<TI>(h, static_cast<const TI*>(X), (int)T, N, mean_out, mask_out, A_out, scale_out);
  });
  API_END(h)
}

int xmca_gap_fill_step(xmca_handle* h, const void* A, const unsigned char* mask, const double* Z, const double* P, int64_t T, int64_t N,
                       int n_modes, int dtype, void* A_out, double* sum_out) {
  API_BEGIN(h)
  XMCA_CHECK(A && mask && Z && P && A_out && sum_out && n_modes >= 1, XMCA_ERR_INVALID, "gap_fill_step: bad arguments");
  check_gap_plane("gap_fill_step", T, N, dtype);
  XMCA_CHECK((int64_t)n_modes * std::max(T, N) < ((int64_t)1 << 34), XMCA_ERR_UNSUPPORTED, "gap_fill_step: coefficient matrices too large");
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    gap_fill_step_impl<TI>(h, static_cast<const TI*>(A), mask, Z, P, (int)T, N, n_modes, static_cast<TI*>(A_out), sum_out);
  });
  API_END(h)
}

int xmca_gap_lag_fill_step(xmca_handle* h, const void* A, const unsigned char* mask, const double* Z, const double* P, int64_t T, int64_t N,
                           int n_modes, int embedding, int tau, int dtype, void* A_out, double* sum_out) {
  API_BEGIN(h)
  XMCA_CHECK(A && mask && Z && P && A_out && sum_out && n_modes >= 1, XMCA_ERR_INVALID, "gap_lag_fill_step: bad arguments");
  check_gap_plane("gap_lag_fill_step", T, N, dtype);
  XMCA_CHECK(embedding >= 1 && tau >= 1, XMCA_ERR_INVALID, "gap_lag_fill_step: embedding and tau must be at least 1");
  const int64_t np = T - (int64_t)(embedding - 1) * tau;
  XMCA_CHECK(np >= 1 && (embedding == 1 || tau <= np), XMCA_ERR_INVALID,
             "gap_lag_fill_step: T - (embedding - 1) * tau must be at least 1, and at least tau when embedding > 1");
  XMCA_CHECK((int64_t)embedding * n_modes * std::max(T, N) < ((int64_t)1 << 34), XMCA_ERR_UNSUPPORTED,
             "gap_lag_fill_step: coefficient matrices too large");
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    gap_lag_fill_step_impl<TI>(h, static_cast<const TI*>(A), mask, Z, P, (int)T, N, n_modes, embedding, tau, static_cast<TI*>(A_out), sum_out);
  });
  API_END(h)
}

int xmca_reg_residual_tile(int* rows_out, int* cols_out) {
  if (!rows_out || !cols_out) return XMCA_ERR_INVALID;
  *rows_out = REG_ROWS;
  *cols_out = REG_COLS;
  return XMCA_OK;
}

// The checks and the call shared by xmca_column_regress (coef == NULL: the fit) and xmca_column_residual
static void column_regress_entry(xmca_handle* h, const char* what, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t,
                                 int64_t stride_n, int dtype, const double* basis, int k, const double* coef, void* field_out, int out_location,
                                 double* coef_out, unsigned char* fitted_out) {
  const std::string w(what);
  XMCA_CHECK(k >= 1 && k <= REG_K, XMCA_ERR_INVALID, w + ": k must lie in [1, 16]");
  XMCA_CHECK(T >= 1 && N >= 1, XMCA_ERR_INVALID, w + ": the field must have at least one row and one column");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, w + ": dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, w + ": strides must not be negative");
  XMCA_CHECK(X && basis && field_out && (coef || (coef_out && fitted_out)), XMCA_ERR_INVALID, w + ": bad arguments");
  XMCA_CHECK(in_location == XMCA_HOST || in_location == XMCA_DEVICE, XMCA_ERR_INVALID, w + ": the location must be XMCA_HOST or XMCA_DEVICE");
  XMCA_CHECK(T <= (int64_t)65535 * REG_ROWS && N < ((int64_t)1 << 31) && T * N < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED, w + ": field too large");
  if (in_location == XMCA_DEVICE) check_device_pointer(h, what, X);
  check_out_location(h, what, out_location, field_out);
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    column_regress_impl<TI>(h, X, in_location == XMCA_DEVICE, (int)T, N, stride_t, stride_n, basis, k, coef, static_cast<TI*>(field_out),
                            out_location == XMCA_DEVICE, coef_out, fitted_out);
  });
}

int xmca_column_regress(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                        const double* basis, int k, void* field_out, int out_location, double* coef_out, unsigned char* fitted_out) {
  API_BEGIN(h)
  XMCA_CHECK(coef_out && fitted_out, XMCA_ERR_INVALID, "column_regress: bad arguments");
  column_regress_entry(h, "column_regress", X, in_location, T, N, stride_t, stride_n, dtype, basis, k, nullptr, field_out, out_location, coef_out,
                       fitted_out);
  API_END(h)
}

int xmca_column_residual(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                         const double* basis, int k, const double* coef, void* field_out, int out_location) {
  API_BEGIN(h)
  XMCA_CHECK(coef, XMCA_ERR_INVALID, "column_residual: bad arguments");
  column_regress_entry(h, "column_residual", X, in_location, T, N, stride_t, stride_n, dtype, basis, k, coef, field_out, out_location, nullptr,
                       nullptr);
  API_END(h)
}

int xmca_time_filter_tile(int* rows_out, int* cols_out, int* max_weights_out) {
  if (!rows_out || !cols_out || !max_weights_out) return XMCA_ERR_INVALID;
  *rows_out = TF_ROWS;
  *cols_out = TF_COLS;
  *max_weights_out = TF_MAX_WEIGHTS;
  return XMCA_OK;
}

int xmca_time_filter(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                     const double* weights, int n_weights, int complement, int renormalise, double den_min, int trim, void* field_out,
                     int out_location) {
  API_BEGIN(h)
  const char* what = "time_filter";
  const std::string w(what);
  XMCA_CHECK(n_weights >= 1 && n_weights <= TF_MAX_WEIGHTS && n_weights % 2 == 1, XMCA_ERR_INVALID,
             w + ": the number of weights must be odd and lie in [1, 1025]");
  XMCA_CHECK(T >= 1 && N >= 1, XMCA_ERR_INVALID, w + ": the field must have at least one row and one column");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, w + ": dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, w + ": strides must not be negative");
  XMCA_CHECK(X && weights && field_out, XMCA_ERR_INVALID, w + ": bad arguments");
  XMCA_CHECK(in_location == XMCA_HOST || in_location == XMCA_DEVICE, XMCA_ERR_INVALID, w + ": the location must be XMCA_HOST or XMCA_DEVICE");
  double sum = 0.0;          // (ascending, as the chain of the denominators: with every entry present den == sum to the bit)
  for (int k = 0; k < n_weights; ++k) {
    XMCA_CHECK(std::isfinite(weights[k]), XMCA_ERR_INVALID, w + ": the weights hold a NaN or an Inf");
    sum += weights[k];
  }
  XMCA_CHECK(!trim || T >= n_weights, XMCA_ERR_INVALID, w + ": trimmed edges need at least as many time steps as weights");
  XMCA_CHECK(!renormalise || !trim, XMCA_ERR_INVALID, w + ": renormalised weights keep the edges, they cannot be trimmed");
  XMCA_CHECK(!renormalise || (sum > 0.0 && den_min > 0.0 && den_min <= sum), XMCA_ERR_INVALID,
             w + ": renormalised weights need a positive sum and 0 < den_min <= that sum");
  XMCA_CHECK(T <= (int64_t)65535 * TF_ROWS && N < ((int64_t)1 << 31) && T * N < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED, w + ": field too large");
  if (in_location == XMCA_DEVICE) check_device_pointer(h, what, X);
  check_out_location(h, what, out_location, field_out);
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    time_filter_impl<TI>(h, X, in_location == XMCA_DEVICE, (int)T, N, stride_t, stride_n, weights, n_weights, complement != 0, renormalise != 0,
                         den_min, trim != 0, static_cast<TI*>(field_out), out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_lead_lag_tile(int* cols_out, int* rows_out, int* lag_group_out) {
  if (!cols_out || !rows_out || !lag_group_out) return XMCA_ERR_INVALID;
  *cols_out = LL_COLS;
  *rows_out = LL_ROWS;
  for (int q = 1; q <= LL_MAX_Q; ++q) lag_group_out[q - 1] = ll_group(q);
  return XMCA_OK;
}

int xmca_lead_lag_maps(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                       const double* Y, int q, const int* lags, int n_lags, int min_pairs, int dof_mode, const double* rho_y, void* r_out,
                       void* slope_out, double* p_out, int* dof_out, int* pairs_out, double* lag1_out, int out_location) {
  API_BEGIN(h)
  const char* what = "lead_lag_maps";
  const std::string w(what);
  XMCA_CHECK(q >= 1 && q <= LL_MAX_Q, XMCA_ERR_INVALID, w + ": between 1 and 8 index series are supported");
  XMCA_CHECK(n_lags >= 1 && (int64_t)n_lags * q <= LL_MAX_ENTRIES, XMCA_ERR_INVALID, w + ": it needs a lag, and at most 1024 lags x index series");
  XMCA_CHECK(T >= 1 && N >= 1, XMCA_ERR_INVALID, w + ": the field must have at least one row and one column");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, w + ": dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, w + ": strides must not be negative");
  XMCA_CHECK(min_pairs >= 3, XMCA_ERR_INVALID, w + ": min_pairs must be at least 3");
  XMCA_CHECK(dof_mode == XMCA_DOF_N || dof_mode == XMCA_DOF_BRETHERTON, XMCA_ERR_INVALID, w + ": dof_mode must be XMCA_DOF_N or XMCA_DOF_BRETHERTON");
  XMCA_CHECK(X && Y && lags && r_out && slope_out && p_out && dof_out && pairs_out, XMCA_ERR_INVALID, w + ": bad arguments");
  XMCA_CHECK(in_location == XMCA_HOST || in_location == XMCA_DEVICE, XMCA_ERR_INVALID, w + ": the location must be XMCA_HOST or XMCA_DEVICE");
  XMCA_CHECK(T <= PVALUE_MAX_OBS, XMCA_ERR_UNSUPPORTED, w + ": T above " + std::to_string(PVALUE_MAX_OBS));
  for (int g = 0; g < n_lags; ++g) {
    XMCA_CHECK((int64_t)lags[g] > -T && (int64_t)lags[g] < T, XMCA_ERR_INVALID, w + ": a lag must lie in [-(T - 1), T - 1]");
    for (int e = 0; e < g; ++e) XMCA_CHECK(lags[e] != lags[g], XMCA_ERR_INVALID, w + ": the lags must be distinct");
  }
  for (int64_t i = 0; i < T * q; ++i) XMCA_CHECK(std::isfinite(Y[i]), XMCA_ERR_INVALID, w + ": the index holds a NaN or an Inf");
  const bool bretherton = dof_mode == XMCA_DOF_BRETHERTON;
  if (bretherton) {
    XMCA_CHECK(rho_y && lag1_out, XMCA_ERR_INVALID, w + ": XMCA_DOF_BRETHERTON needs rho_y and lag1_out");
    for (int j = 0; j < q; ++j) XMCA_CHECK(rho_y[j] >= -1.0 && rho_y[j] <= 1.0, XMCA_ERR_INVALID, w + ": rho_y must lie in [-1, 1]");
  }
  XMCA_CHECK(N < ((int64_t)1 << 31) && T * N < ((int64_t)1 << 40) && (int64_t)n_lags * N * ll_moments(q) < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED,
             w + ": field too large");
  if (in_location == XMCA_DEVICE) check_device_pointer(h, what, X);
  check_out_location(h, what, out_location, r_out);
  if (out_location == XMCA_DEVICE) {
    check_device_pointer(h, what, slope_out);
    check_device_pointer(h, what, p_out);
    check_device_pointer(h, what, dof_out);
    check_device_pointer(h, what, pairs_out);
    if (bretherton) check_device_pointer(h, what, lag1_out);
  }
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    lead_lag_impl<TI>(h, X, in_location == XMCA_DEVICE, (int)T, N, stride_t, stride_n, Y, q, lags, n_lags, min_pairs, bretherton, rho_y,
                      static_cast<TI*>(r_out), static_cast<TI*>(slope_out), p_out, dof_out, pairs_out, lag1_out, out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_spectral_tile(int* cols_out, int* rows_out, int* bin_group_out) {
  if (!cols_out || !rows_out || !bin_group_out) return XMCA_ERR_INVALID;
  *cols_out = SP_COLS;
  *rows_out = SP_ROWS;
  for (int q = 0; q <= SP_MAX_Q; ++q) bin_group_out[q] = sp_group(q);
  return XMCA_OK;
}

int xmca_spectral_maps(xmca_handle* h, const void* X, int in_location, int64_t T, int64_t N, int64_t stride_t, int64_t stride_n, int dtype,
                       const double* Y, int q, int nperseg, int step, const double* weights, int detrend, const int* bins, int n_bins, double fs,
                       int min_segments, void* power_out, void* index_power_out, void* cospectrum_out, void* quadrature_out, void* coherence_out,
                       void* phase_out, void* gain_out, double* p_out, int* segments_out, int out_location) {
  API_BEGIN(h)
  const char* what = "spectral_maps";
  const std::string w(what);
  const int L = nperseg;
  XMCA_CHECK(q >= 0 && q <= SP_MAX_Q, XMCA_ERR_INVALID, w + ": between 0 and 4 index series are supported");
  XMCA_CHECK(T >= 1 && N >= 1, XMCA_ERR_INVALID, w + ": the field must have at least one row and one column");
  XMCA_CHECK(L >= SP_MIN_L && L <= SP_MAX_L && L <= T, XMCA_ERR_INVALID, w + ": nperseg must lie in [8, 4096] and not exceed T");
  XMCA_CHECK(step >= (L + 3) / 4 && step <= L, XMCA_ERR_INVALID, w + ": step must lie in [ceil(nperseg / 4), nperseg]");
  XMCA_CHECK(detrend == XMCA_DETREND_NONE || detrend == XMCA_DETREND_MEAN, XMCA_ERR_INVALID, w + ": detrend must be XMCA_DETREND_NONE or XMCA_DETREND_MEAN");
  XMCA_CHECK(n_bins >= 1 && n_bins <= L / 2 + 1, XMCA_ERR_INVALID, w + ": between 1 and nperseg / 2 + 1 bins");
  XMCA_CHECK(std::isfinite(fs) && fs > 0.0, XMCA_ERR_INVALID, w + ": fs must be positive and finite");
  XMCA_CHECK(min_segments >= 1, XMCA_ERR_INVALID, w + ": min_segments must be at least 1");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, w + ": dtype must be XMCA_F32 or XMCA_F64");
  XMCA_CHECK(stride_t >= 0 && stride_n >= 0, XMCA_ERR_INVALID, w + ": strides must not be negative");
  XMCA_CHECK(X && weights && bins && power_out && segments_out, XMCA_ERR_INVALID, w + ": bad arguments");
  XMCA_CHECK(q == 0 || (Y && index_power_out && cospectrum_out && quadrature_out && coherence_out && phase_out && gain_out && p_out), XMCA_ERR_INVALID,
             w + ": an index needs its series and every one of its maps");
  XMCA_CHECK(in_location == XMCA_HOST || in_location == XMCA_DEVICE, XMCA_ERR_INVALID, w + ": the location must be XMCA_HOST or XMCA_DEVICE");
  {
    std::vector<char> seen((size_t)L / 2 + 1, 0);
    for (int f = 0; f < n_bins; ++f) {
      XMCA_CHECK(bins[f] >= 0 && bins[f] <= L / 2, XMCA_ERR_INVALID, w + ": a bin must lie in [0, nperseg / 2]");
      XMCA_CHECK(!seen[(size_t)bins[f]], XMCA_ERR_INVALID, w + ": the bins must be distinct");
      seen[(size_t)bins[f]] = 1;
    }
  }
  double w2 = 0.0;
  for (int i = 0; i < L; ++i) {
    XMCA_CHECK(std::isfinite(weights[i]), XMCA_ERR_INVALID, w + ": the weights hold a NaN or an Inf");
    w2 += weights[i] * weights[i];
  }
  XMCA_CHECK(w2 > 0.0 && std::isfinite(w2), XMCA_ERR_INVALID, w + ": the sum of the squared weights must be positive and finite");
  for (int64_t i = 0; i < T * q; ++i) XMCA_CHECK(std::isfinite(Y[i]), XMCA_ERR_INVALID, w + ": the index holds a NaN or an Inf");
  XMCA_CHECK(N < ((int64_t)1 << 31) && T < ((int64_t)1 << 31) && T * N < ((int64_t)1 << 40) && (int64_t)n_bins * N * sp_sums(q) < ((int64_t)1 << 40),
             XMCA_ERR_UNSUPPORTED, w + ": field too large");
  if (in_location == XMCA_DEVICE) check_device_pointer(h, what, X);
  check_out_location(h, what, out_location, power_out);
  if (out_location == XMCA_DEVICE) {
    check_device_pointer(h, what, segments_out);
    if (q > 0) {
      for (const void* ptr : {(const void*)index_power_out, (const void*)cospectrum_out, (const void*)quadrature_out, (const void*)coherence_out,
                              (const void*)phase_out, (const void*)gain_out, (const void*)p_out})
        check_device_pointer(h, what, ptr);
    }
  }
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    spectral_impl<TI>(h, X, in_location == XMCA_DEVICE, (int)T, N, stride_t, stride_n, Y, q, L, step, weights, detrend == XMCA_DETREND_MEAN, bins,
                      n_bins, fs, min_segments, static_cast<TI*>(power_out), static_cast<TI*>(index_power_out), static_cast<TI*>(cospectrum_out),
                      static_cast<TI*>(quadrature_out), static_cast<TI*>(coherence_out), static_cast<TI*>(phase_out), static_cast<TI*>(gain_out), p_out,
                      segments_out, out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_reg_mask(xmca_handle* h, const void* X, int64_t T, int64_t N, int dtype, unsigned char* mask_out, double* wide_out,
                  int64_t* missing_out) {
  API_BEGIN(h)
  XMCA_CHECK(X && mask_out && wide_out && missing_out, XMCA_ERR_INVALID, "reg_mask: bad arguments");
  check_gap_plane("reg_mask", T, N, dtype);
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    reg_mask_impl<TI>(h, static_cast<const TI*>(X), T * N, mask_out, wide_out, missing_out);
  });
  API_END(h)
}

int xmca_reg_solve(xmca_handle* h, const double* normal, int shared_normal, const double* rhs, int64_t N, int k, double* coef_out,
                   unsigned char* fitted_out) {
  API_BEGIN(h)
  XMCA_CHECK(k >= 1 && k <= REG_K, XMCA_ERR_INVALID, "reg_solve: k must lie in [1, 16]");
  XMCA_CHECK(normal && rhs && coef_out && fitted_out && N >= 1 && N < ((int64_t)1 << 31), XMCA_ERR_INVALID, "reg_solve: bad arguments");
  reg_solve_impl(h, normal, shared_normal != 0, rhs, N, k, coef_out, fitted_out);
  API_END(h)
}

int xmca_extended_reconstruct(xmca_handle* h, int embedding, int tau, const int* modes, int n_sel, int add_means, const int64_t* keep_idx,
                              int64_t N_keep, int64_t N_full, const double* mean, const double* stdv, const double* inv_weight, double* out,
                              int out_location) {
  API_BEGIN(h)
  const int64_t np = check_lag_embedding(h, "extended_reconstruct", embedding, tau, 2);
  const int64_t T = resident_T(h), N = resident_N(h, 0);
  XMCA_CHECK(embedding == 1 || tau <= np, XMCA_ERR_INVALID,
             "extended_reconstruct: tau above T' leaves time steps outside every window (no reconstruction there)");
  XMCA_CHECK(modes && n_sel >= 1 && out, XMCA_ERR_INVALID, "extended_reconstruct: need at least one mode and an output");
  const int64_t most = std::min<int64_t>(np - 1, (int64_t)embedding * N);
  for (int c = 0; c < n_sel; ++c)
    XMCA_CHECK(modes[c] >= 0 && modes[c] < most && (c == 0 || modes[c] > modes[c - 1]), XMCA_ERR_INVALID,
               "extended_reconstruct: modes must be increasing 0-based indices below min(T' - 1, embedding * N)");
  XMCA_CHECK(N_keep == N, XMCA_ERR_INVALID, "extended_reconstruct: N_keep must be the field's " + std::to_string(N) + " columns");
  check_kept_columns("extended_reconstruct", keep_idx, N, N_full, INT32_MAX);
  const int64_t kin = (int64_t)embedding * (n_sel + 1);
  XMCA_CHECK(kin <= INT32_MAX && kin * std::max(N, T) < ((int64_t)1 << 40), XMCA_ERR_UNSUPPORTED,
             "extended_reconstruct: coefficient matrices too large");
  check_out_location(h, "extended_reconstruct", out_location, out);
  with_dtype(h->dtype, [&](auto t) {
    extended_reconstruct_impl<decltype(t)>(h, embedding, tau, modes, n_sel, add_means != 0, keep_idx, N_full, mean, stdv, inv_weight, out,
                                           out_location == XMCA_DEVICE);
  });
  API_END(h)
}

int xmca_lag_expand(xmca_handle* h, const double* Z, int q, int Tp, int embedding, int tau, int with_indicators, double* A_out,
                    double* inv_count_out) {
  API_BEGIN(h)
  XMCA_CHECK(Z && A_out && inv_count_out && q >= 1 && Tp >= 1 && embedding >= 1 && tau >= 1, XMCA_ERR_INVALID, "lag_expand: bad arguments");
  XMCA_CHECK(embedding == 1 || tau <= Tp, XMCA_ERR_INVALID, "lag_expand: tau above T' leaves time steps outside every window");
  const int64_t T = (int64_t)Tp + (int64_t)(embedding - 1) * tau, kin = (int64_t)embedding * (q + (with_indicators ? 1 : 0));
  check_operator_size("lag_expand", T);
  XMCA_CHECK(kin <= INT32_MAX && kin * T < ((int64_t)1 << 34) && (int64_t)q * Tp < ((int64_t)1 << 34), XMCA_ERR_UNSUPPORTED,
             "lag_expand: coefficient matrix too large");
  DevBuf<double> Zd, A, inv_count;
  XMCA_HIP(hipMemcpyAsync(Zd.ensure((size_t)q * Tp), Z, sizeof(double) * (size_t)q * Tp, hipMemcpyHostToDevice, h->st));
  h->tm.begin("eeof_expand");
  lag_expand(h->st, Zd.get(), q, Tp, embedding, tau, with_indicators != 0, A.ensure((size_t)(T * kin)), inv_count.ensure((size_t)T));
  h->tm.end();
  XMCA_HIP(hipMemcpyAsync(A_out, A.get(), sizeof(double) * (size_t)(T * kin), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(inv_count_out, inv_count.get(), sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_lag_window_means(xmca_handle* h, int embedding, int tau, double* means_out) {
  API_BEGIN(h)
  check_lag_embedding(h, "lag_window_means", embedding, tau, 1);
  XMCA_CHECK(means_out && resident_N(h, 0) < ((int64_t)1 << 31), XMCA_ERR_INVALID, "lag_window_means: bad arguments");
  with_dtype(h->dtype, [&](auto t) { lag_window_means_impl<decltype(t)>(h, embedding, tau, means_out); });
  API_END(h)
}

// the checks of xmca_extended_eofs that the Monte-Carlo SSA entries share (its errors, in its order)
static void check_mcssa(xmca_handle* h, const char* what, bool outputs, int embedding, int tau, int n_modes) {
  const std::string w(what);
  XMCA_CHECK(!h->field_set[0] || (outputs && n_modes >= 1), XMCA_ERR_INVALID, w + ": bad arguments");
  const int64_t np = check_lag_embedding(h, what, embedding, tau, 2);
  const int64_t T = resident_T(h), N = resident_N(h, 0);
  XMCA_CHECK(n_modes <= np - 1 && n_modes <= (int64_t)embedding * N, XMCA_ERR_INVALID,
             w + ": n_modes must not exceed min(T' - 1, embedding * N)");
  XMCA_CHECK(N < ((int64_t)1 << 31) && (int64_t)embedding * n_modes * std::max(N, T) < ((int64_t)1 << 40) &&
                 (int64_t)embedding * n_modes <= INT32_MAX,
             XMCA_ERR_UNSUPPORTED, w + ": pattern array too large");
}

int xmca_extended_rule_n(xmca_handle* h, int embedding, int tau, int n_modes, const double* phi, int64_t run_begin, int64_t run_end,
                         uint64_t seed, double* lam_out, double* scale_out, double* surrogates_out) {
  API_BEGIN(h)
  check_mcssa(h, "extended_rule_n", lam_out && scale_out && surrogates_out, embedding, tau, n_modes);
  XMCA_CHECK(run_begin >= 0 && run_end >= run_begin && run_end <= (int64_t)UINT32_MAX && (run_end - run_begin) * n_modes < ((int64_t)1 << 34),
             XMCA_ERR_INVALID, "extended_rule_n: bad run range");
  check_phi("extended_rule_n", phi, resident_N(h, 0));
  with_dtype(h->dtype, [&](auto t) {
    extended_rule_n_impl<decltype(t)>(h, embedding, tau, n_modes, phi, run_begin, run_end, seed, lam_out, scale_out, surrogates_out);
  });
  h->tm.collect();
  API_END(h)
}

int xmca_extended_project(xmca_handle* h, int embedding, int tau, int n_modes, const double* R, int apply_scale, double* out) {
  API_BEGIN(h)
  check_mcssa(h, "extended_project", R && out, embedding, tau, n_modes);
  with_dtype(h->dtype, [&](auto t) { extended_project_impl<decltype(t)>(h, embedding, tau, n_modes, R, apply_scale != 0, out); });
  API_END(h)
}

int xmca_lag_project(xmca_handle* h, const double* W, int64_t T, int embedding, int tau, int k, double* out) {
  API_BEGIN(h)
  XMCA_CHECK(W && out && T >= 1 && embedding >= 1 && tau >= 1 && k >= 1, XMCA_ERR_INVALID, "lag_project: bad arguments");
  check_operator_size("lag_project", T);
  XMCA_CHECK(T - (int64_t)(embedding - 1) * tau >= 1, XMCA_ERR_INVALID, "lag_project: (embedding - 1) * tau must be below T");
  XMCA_CHECK((int64_t)embedding * k <= INT32_MAX && (int64_t)embedding * k * T < ((int64_t)1 << 34), XMCA_ERR_UNSUPPORTED,
             "lag_project: matrix too large");
  lag_project_impl(h, W, (int)T, embedding, tau, k, out);
  API_END(h)
}

int xmca_lag_project_tile(int* rows_out, int* cols_out) {
  if (!rows_out || !cols_out) return XMCA_ERR_INVALID;
  *rows_out = LAGP_ROWS;
  *cols_out = LAGP_COLS;
  return XMCA_OK;
}

int xmca_correlate(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, double* r_out) {
  API_BEGIN(h)
  check_side("correlate", side);
  XMCA_CHECK(h->field_set[side], XMCA_ERR_STATE, "correlate: no field resident for this side");
  XMCA_CHECK(Y && r_out && T >= 2 && m >= 1, XMCA_ERR_INVALID, "correlate: need a T x m matrix");
  with_dtype(h->dtype, [&](auto t) { correlate_impl<decltype(t)>(h, side, Y, T, m, r_out); });
  API_END(h)
}

int xmca_pvalue_log_norm(int64_t n_obs, double* out) {
  if (!out || n_obs < 3 || n_obs > PVALUE_MAX_OBS) return XMCA_ERR_INVALID;
  *out = pvalue_log_norm(n_obs);
  return XMCA_OK;
}

int xmca_pearson_pvalues(xmca_handle* h, const double* r, int64_t count, int64_t n_obs, double* p_out) {
  API_BEGIN(h)
  XMCA_CHECK(n_obs >= 3, XMCA_ERR_INVALID, "pearson_pvalues: the null distribution needs n_obs >= 3");
  XMCA_CHECK(n_obs <= PVALUE_MAX_OBS, XMCA_ERR_UNSUPPORTED, "pearson_pvalues: n_obs above " + std::to_string(PVALUE_MAX_OBS));
  XMCA_CHECK(count >= 0 && (count == 0 || (r && p_out)), XMCA_ERR_INVALID, "pearson_pvalues: need `count` values and an output");
  if (count > 0) pearson_pvalues_impl(h, r, count, n_obs, p_out);
  API_END(h)
}

int xmca_correlation_maps(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, const int64_t* keep_idx, int64_t N_full,
                          int r_dtype, void* r_out, double* p_out) {
  return xmca_correlation_maps_to(h, side, Y, T, m, keep_idx, N_full, r_dtype, r_out, p_out, XMCA_HOST);
}

int xmca_correlation_maps_to(xmca_handle* h, int side, const double* Y, int64_t T, int64_t m, const int64_t* keep_idx, int64_t N_full,
                             int r_dtype, void* r_out, double* p_out, int out_location) {
  API_BEGIN(h)
  check_side("correlation_maps", side);
  XMCA_CHECK(h->field_set[side], XMCA_ERR_STATE, "correlation_maps: no field resident for this side");
  XMCA_CHECK(Y && r_out && p_out && m >= 1 && m <= INT32_MAX, XMCA_ERR_INVALID, "correlation_maps: need a T x m matrix and two outputs");
  XMCA_CHECK(T >= 3, XMCA_ERR_INVALID, "correlation_maps: the null distribution needs T >= 3");
  XMCA_CHECK(T <= PVALUE_MAX_OBS, XMCA_ERR_UNSUPPORTED, "correlation_maps: T above " + std::to_string(PVALUE_MAX_OBS));
  XMCA_CHECK(r_dtype == XMCA_F32 || r_dtype == XMCA_F64, XMCA_ERR_INVALID, "correlation_maps: r_dtype must be XMCA_F32 or XMCA_F64");
  check_out_location(h, "correlation_maps", out_location, r_out);
  check_out_location(h, "correlation_maps", out_location, p_out);
  check_kept_columns("correlation_maps", keep_idx, resident_N(h, side), N_full, INT32_MAX);
  with_dtype(h->dtype, [&](auto t) {
    with_dtype(r_dtype, [&](auto tr) {
      correlation_maps_impl<decltype(t), decltype(tr)>(h, side, Y, T, m, keep_idx, N_full, static_cast<decltype(tr)*>(r_out), p_out,
                                                       out_location == XMCA_DEVICE);
    });
  });
  API_END(h)
}

int xmca_rotate_loadings(xmca_handle* h, const double* L, int64_t N, int64_t n_left, int p, int is_complex, int power,
                         double tol, int max_iter, int varimax_only, double gamma, double* B_out, double* R_out, double* Phi_out,
                         double* norm_left, double* norm_right, int* iters_out) {
  API_BEGIN_NO_JOIN(h)
  // The loadings come from the host and the rotation reads nothing of the solve.  On the fourth-moment route (real, few modes) its
  // loop is ONE workgroup: it runs beside the tail.  Every other route joins: a persistent grid, whose workgroups wait for each
  // other, must not queue for CUs behind the tail's workgroups, and the GEMM-based route would share the chip with it for nothing.
  if (!Rotator::single_workgroup_loop(p, is_complex != 0)) join_tail(h);
  XMCA_CHECK(L && N >= 1 && p >= 2, XMCA_ERR_INVALID, "rotate: need N x p loadings with p >= 2");
  XMCA_CHECK(power >= 1, XMCA_ERR_INVALID, "rotate: `power` must be >= 1");
  XMCA_CHECK(n_left >= 0 && n_left <= N && max_iter >= 1, XMCA_ERR_INVALID, "rotate: bad n_left / max_iter");
  const bool cplx = is_complex != 0;
  Rotator rot(h->st, h->tm, h->gws, h->ews);
  rot.gamma = gamma;
  RotationDevice& d = h->rot;
  rot.alloc(d, N, n_left, p, cplx);
  const size_t nl = (size_t)N * p * (cplx ? 2 : 1);
  DevBuf<double> Ld, Bd;
  XMCA_HIP(hipMemcpyAsync(Ld.ensure(nl), L, sizeof(double) * nl, hipMemcpyHostToDevice, h->st));
  if (B_out) Bd.ensure(nl);
  RotateResult rr;
  if (cplx) {
    hipLaunchKernelGGL((rot_import_loadings_kernel<true>), ew_grid(N), dim3(EW_BLOCK), 0, h->st, Ld.get(), N, p, d.A.r(), d.A.i(true),
                       d.h.get());
  } else {
    hipLaunchKernelGGL((rot_import_loadings_kernel<false>), ew_grid(N), dim3(EW_BLOCK), 0, h->st, Ld.get(), N, p, d.A.r(),
                       (double*)nullptr, d.h.get());
  }
  rot.run(d, power, tol, max_iter, rr, B_out ? Bd.get() : nullptr, varimax_only != 0);
  h->tm.collect();
  if (iters_out) *iters_out = rr.iters;
  check_rot(rr);
  fill_rot_outputs(rr, cplx, R_out, Phi_out, norm_left, norm_right, iters_out);
  if (B_out) {
    XMCA_HIP(hipMemcpyAsync(B_out, Bd.get(), sizeof(double) * nl, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
  }
  API_END(h)
}

int xmca_rotate_solved(xmca_handle* h, int p, int power, double tol, int max_iter, double* R_out, double* Phi_out,
                       double* norm_left, double* norm_right, int* iters_out) {
  API_BEGIN_NO_JOIN(h)
  if (!h->solved) join_tail(h);       // (no tail is pending without a result; an entry point joins unless it says why not)
  XMCA_CHECK(h->solved, XMCA_ERR_STATE, "rotate: no solve result on this handle");
  // The rule of xmca_rotate_loadings: on the fourth-moment route (real, few modes) the loop is one workgroup and runs beside the
  // tail, provided the loadings come from modes that were complete when solve returned - the first tail.head rows of the
  // plane (float64 or float32) on the head / tail route, tail.lead_modes() on the lead route; every other case joins.
  if (!(Rotator::single_workgroup_loop(p, h->res.cplx) && p <= h->tail.head)) join_tail(h);
  XMCA_CHECK(p >= 2, XMCA_ERR_INVALID, "rotate: `n_rot` must be > 1");
  XMCA_CHECK(power >= 1 && max_iter >= 1, XMCA_ERR_INVALID, "rotate: `power` must be >= 1");
  const SolveResult& r = h->res;
  XMCA_CHECK(p <= r.n_vec && r.ldv[0] > 0, XMCA_ERR_INVALID, "rotate: more modes requested than were back-projected");
  const bool cplx = r.cplx;
  Rotator rot(h->st, h->tm, h->gws, h->ews);
  DevBuf<double> sigma_dev;
  RotateResult rr;
  rotate_resident(h, rot, h->rot, sigma_dev, r, r.ldv[0], r.ldv[1] > 0 ? r.ldv[1] : 0, p, power, tol, max_iter, rr, h->tail.lead_modes());
  h->tm.collect();
  if (iters_out) *iters_out = rr.iters;
  check_rot(rr);
  fill_rot_outputs(rr, cplx, R_out, Phi_out, norm_left, norm_right, iters_out);
  API_END(h)
}

// xmca_rule_n (ar1 == false: white surrogates, phi_* unused) and xmca_rule_n_ar1 (phi_left, and phi_right for two fields)
static int rule_n_entry(xmca_handle* h, int64_t T, int64_t Nx, int64_t Ny, int n_fields, const double* hilbert_col, int rotated, int p,
                        int power, double tol, int64_t run_begin, int64_t run_end, uint64_t seed, int dtype, double* spectra_out,
                        int* kept_out, int64_t n_out, bool ar1, const double* phi_left, const double* phi_right) {
  API_BEGIN(h)
  XMCA_CHECK(n_fields == 1 || n_fields == 2, XMCA_ERR_INVALID, "rule_n: n_fields must be 1 or 2");
  XMCA_CHECK(T >= 2 && Nx >= 1 && (n_fields == 1 || Ny >= 1), XMCA_ERR_INVALID, "rule_n: bad field shape");
  XMCA_CHECK(run_end >= run_begin && spectra_out && kept_out, XMCA_ERR_INVALID, "rule_n: bad run range / outputs");
  check_rotation_args("rule_n", "bad rotation parameters", rotated, p, power);
  ComplexOp hop;
  if (hilbert_col) hop = ComplexOp::circulant(hilbert_col, T);
  const ReplicateSpec spec{T, Nx, Ny, n_fields, hilbert_col ? &hop : nullptr, rotated, p, power, tol};
  // phi goes up once, before the lanes start; they only read it
  DevBuf<double> phi_dev[2];
  const double* phi[2] = {nullptr, nullptr};
  if (ar1) {
    const double* phi_host[2] = {phi_left, phi_right};
    const int64_t Ns[2] = {Nx, Ny};
    XMCA_CHECK(n_fields == 2 || !phi_right, XMCA_ERR_INVALID, "rule_n_ar1: phi_right given for a model of one field");
    for (int s = 0; s < n_fields; ++s) check_phi("rule_n_ar1", phi_host[s], Ns[s]);
    for (int s = 0; s < n_fields; ++s) {
      XMCA_HIP(hipMemcpyAsync(phi_dev[s].ensure((size_t)Ns[s]), phi_host[s], sizeof(double) * Ns[s], hipMemcpyHostToDevice, h->st));
      phi[s] = phi_dev[s].get();
    }
    XMCA_HIP(hipStreamSynchronize(h->st));
  }
  with_dtype(dtype, [&](auto t) {
    rule_n_impl<decltype(t)>(h, spec, run_begin, run_end, seed, spectra_out, kept_out, n_out, ar1 ? phi : nullptr);
  });
  h->tm.collect();
  API_END(h)
}

int xmca_rule_n(xmca_handle* h, int64_t T, int64_t Nx, int64_t Ny, int n_fields, const double* hilbert_col, int rotated,
                int p, int power, double tol, int64_t run_begin, int64_t run_end, uint64_t seed, int dtype,
                double* spectra_out, int* kept_out, int64_t n_out) {
  return rule_n_entry(h, T, Nx, Ny, n_fields, hilbert_col, rotated, p, power, tol, run_begin, run_end, seed, dtype, spectra_out, kept_out,
                      n_out, false, nullptr, nullptr);
}

int xmca_rule_n_ar1(xmca_handle* h, int64_t T, int64_t Nx, int64_t Ny, int n_fields, const double* hilbert_col, int rotated,
                    int p, int power, double tol, int64_t run_begin, int64_t run_end, uint64_t seed, int dtype,
                    double* spectra_out, int* kept_out, int64_t n_out, const double* phi_left, const double* phi_right) {
  return rule_n_entry(h, T, Nx, Ny, n_fields, hilbert_col, rotated, p, power, tol, run_begin, run_end, seed, dtype, spectra_out, kept_out,
                      n_out, true, phi_left, phi_right);
}

int xmca_lag1_autocorrelation(xmca_handle* h, int side, double* phi_out) {
  API_BEGIN(h)
  check_side("lag1_autocorrelation", side);
  XMCA_CHECK(phi_out, XMCA_ERR_INVALID, "lag1_autocorrelation: no output");
  XMCA_CHECK(h->field_set[side], XMCA_ERR_STATE, "lag1_autocorrelation: set the field first");
  with_dtype(h->dtype, [&](auto t) { lag1_impl<decltype(t)>(h, side, phi_out); });
  API_END(h)
}

int xmca_ar1_segments(int64_t T, int64_t N, int64_t* count_out, int64_t* length_out) {
  if (T < 1 || N < 1 || !count_out || !length_out) return XMCA_ERR_INVALID;
  const ::xmca::Ar1Segments seg = ::xmca::ar1_segments(T, N);
  *count_out = seg.count;
  *length_out = seg.length;
  return XMCA_OK;
}

int xmca_surrogate_ar1(xmca_handle* h, int64_t T, int64_t N, const double* phi, uint64_t seed, uint32_t run, uint32_t side, int dtype,
                       double* out) {
  API_BEGIN(h)
  XMCA_CHECK(T >= 1 && N >= 1 && out, XMCA_ERR_INVALID, "surrogate_ar1: bad arguments");
  XMCA_CHECK(dtype == XMCA_F32 || dtype == XMCA_F64, XMCA_ERR_INVALID, "surrogate_ar1: dtype must be XMCA_F32 or XMCA_F64");
  check_phi("surrogate_ar1", phi, N);
  with_dtype(dtype, [&](auto t) { surrogate_ar1_impl<decltype(t)>(h, T, N, phi, seed, run, side, out); });
  API_END(h)
}

// ---- RCCL communicator (comm.h) ----------------------------------------------------------------------------------
#define COMM_BEGIN(c)                                                  \
  if (!(c)) return XMCA_ERR_INVALID;                                   \
  try {                                                                \
    XMCA_HIP(hipSetDevice((c)->device));
#define COMM_END(c) } XMCA_CATCH(c)

int xmca_comm_unique_id(void* id_out) {
  if (!id_out) return XMCA_ERR_INVALID;
  RcclApi& api = RcclApi::get();
  if (!api.lib) return XMCA_ERR_UNSUPPORTED;
  ncclUniqueId id;
  if (api.GetUniqueId(&id) != ncclSuccess) return XMCA_ERR_HIP;
  std::memcpy(id_out, id.internal, XMCA_COMM_ID_BYTES);
  return XMCA_OK;
}

int xmca_comm_create(xmca_handle* h, const void* unique_id, int rank, int world, xmca_comm** out) {
  if (!out) return XMCA_ERR_INVALID;
  *out = nullptr;
  API_BEGIN(h)
  XMCA_CHECK(unique_id && world >= 1 && rank >= 0 && rank < world, XMCA_ERR_INVALID, "comm_create: bad rank / world / id");
  RcclApi& api = RcclApi::get();
  api.require();
  xmca_comm* c = new xmca_comm();
  c->device = h->device;
  c->rank = rank;
  c->world = world;
  try {
    XMCA_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    ncclUniqueId id;
    std::memcpy(id.internal, unique_id, XMCA_COMM_ID_BYTES);
    api.check(api.CommInitRank(&c->comm, world, id, rank), "ncclCommInitRank");
  } catch (...) {
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
    throw;
  }
  *out = c;
  API_END(h)
}

void xmca_comm_destroy(xmca_comm* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->st) (void)hipStreamSynchronize(c->st);
  RcclApi& api = RcclApi::get();
  if (c->comm && api.lib) (void)api.CommDestroy(c->comm);
  c->send.release();
  c->recv.release();
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

const char* xmca_comm_last_error(xmca_comm* c) { return c ? c->err.c_str() : "null communicator"; }

int xmca_comm_allgather(xmca_comm* c, const double* send_host, double* recv_host, int64_t count) {
  COMM_BEGIN(c)
  XMCA_CHECK(count >= 0 && (count == 0 || (send_host && recv_host)), XMCA_ERR_INVALID, "comm_allgather: bad arguments");
  if (count > 0) {
    RcclApi& api = RcclApi::get();
    api.require();
    double* s = c->send.ensure((size_t)count);
    double* r = c->recv.ensure((size_t)count * c->world);
    XMCA_HIP(hipMemcpyAsync(s, send_host, sizeof(double) * count, hipMemcpyHostToDevice, c->st));
    api.check(api.AllGather(s, r, (size_t)count, ncclFloat64, c->comm, c->st), "ncclAllGather");
    XMCA_HIP(hipMemcpyAsync(recv_host, r, sizeof(double) * count * c->world, hipMemcpyDeviceToHost, c->st));
    XMCA_HIP(hipStreamSynchronize(c->st));
    c->collectives += 1;
    c->bytes += (long long)sizeof(double) * count * c->world;
  }
  COMM_END(c)
}

int xmca_comm_broadcast(xmca_comm* c, double* buf_host, int64_t count, int root) {
  COMM_BEGIN(c)
  XMCA_CHECK(count >= 0 && (count == 0 || buf_host) && root >= 0 && root < c->world, XMCA_ERR_INVALID, "comm_broadcast: bad arguments");
  if (count > 0) {
    RcclApi& api = RcclApi::get();
    api.require();
    double* s = c->send.ensure((size_t)count);
    XMCA_HIP(hipMemcpyAsync(s, buf_host, sizeof(double) * count, hipMemcpyHostToDevice, c->st));
    api.check(api.Broadcast(s, s, (size_t)count, ncclFloat64, root, c->comm, c->st), "ncclBroadcast");
    XMCA_HIP(hipMemcpyAsync(buf_host, s, sizeof(double) * count, hipMemcpyDeviceToHost, c->st));
    XMCA_HIP(hipStreamSynchronize(c->st));
    c->collectives += 1;
    c->bytes += (long long)sizeof(double) * count;
  }
  COMM_END(c)
}

int xmca_comm_info(xmca_comm* c, int* rank, int* world, int64_t* collectives, int64_t* bytes) {
  if (!c) return XMCA_ERR_INVALID;
  if (rank) *rank = c->rank;
  if (world) *world = c->world;
  if (collectives) *collectives = c->collectives;
  if (bytes) *bytes = c->bytes;
  return XMCA_OK;
}

// Shard, all-gather and status row of xmca_rule_n_sharded / xmca_rule_n_ar1_sharded: local(b, e, seed, spectra, kept) runs this
// rank's block [b, e) of the runs with the seed of rank 0 and returns its status
static int rule_n_sharded_body(xmca_handle* h, xmca_comm* c, int64_t n_runs, uint64_t seed, double* spectra_out, int* kept_out,
                               int64_t n_out, const std::function<int(int64_t, int64_t, uint64_t, double*, int*)>& local_runs) {
  if (!h || !c) return XMCA_ERR_INVALID;
  if (n_runs < 0 || n_out < 1 || !spectra_out || !kept_out) { h->err = "rule_n_sharded: bad arguments"; return XMCA_ERR_INVALID; }
  if (c->device != h->device) { h->err = "rule_n_sharded: the communicator belongs to another device"; return XMCA_ERR_INVALID; }
  // the seed of rank 0 keys every rank's generator (two 32-bit halves: exact in float64)
  double sd[2] = {(double)(uint32_t)(seed & 0xffffffffu), (double)(uint32_t)(seed >> 32)};
  int rc = xmca_comm_broadcast(c, sd, 2, 0);
  if (rc != XMCA_OK) { h->err = "rule_n_sharded: " + c->err; return rc; }
  seed = (uint64_t)(uint32_t)sd[0] | ((uint64_t)(uint32_t)sd[1] << 32);
  // contiguous blocks whose sizes differ by at most one (xmca_amd/dist.py shard_range)
  const int64_t world = c->world, base = n_runs / world, rem = n_runs % world;
  auto begin_of = [&](int64_t r) { return r * base + std::min<int64_t>(r, rem); };
  const int64_t b = begin_of(c->rank), e = begin_of(c->rank + 1);
  const int64_t cap = base + (rem ? 1 : 0);
  // Payload of a rank: its `cap` rows of (n_out spectra, kept) and ONE status row (status code, 0...).  A rank whose own
  // runs failed (out of memory, a device error, a lane error) STILL enters the all-gather - with its status - so that no rank is
  // left waiting in the collective; afterwards every rank returns the same error (round 6; advisor / VERDICT r05: the early
  // return here left the other ranks in ncclAllGather for good).  A rank without runs (world > n_runs) validates the
  // arguments through an empty range: a bad-argument failure is the same on every rank.
  const int64_t rows = cap + 1, width = n_out + 1;
  std::vector<double> local((size_t)rows * width, 0.0), all;
  std::vector<double> sp((size_t)std::max<int64_t>(e - b, 1) * n_out, 0.0);
  std::vector<int> kp((size_t)std::max<int64_t>(e - b, 1), 0);
  int local_rc = local_runs(b, e, seed, sp.data(), kp.data());
  if (const char* inj = std::getenv("XMCA_TEST_FAIL_RANK"))          // (tests: make this rank's shard fail)
    if (std::atoi(inj) == c->rank && local_rc == XMCA_OK) { local_rc = XMCA_ERR_NUMERIC; h->err = "rule_n_sharded: injected failure (XMCA_TEST_FAIL_RANK)"; }
  const std::string local_err = h->err;
  if (local_rc == XMCA_OK) {
    for (int64_t i = 0; i < e - b; ++i) {
      std::memcpy(&local[(size_t)i * width], &sp[(size_t)i * n_out], sizeof(double) * n_out);
      local[(size_t)i * width + n_out] = (double)kp[(size_t)i];
    }
  }
  local[(size_t)cap * width] = (double)local_rc;
  all.assign((size_t)rows * width * world, 0.0);
  rc = xmca_comm_allgather(c, local.data(), all.data(), rows * width);
  if (rc != XMCA_OK) { h->err = "rule_n_sharded: " + c->err + (local_rc != XMCA_OK ? " (and this rank's shard failed: " + local_err + ")" : ""); return rc; }
  int first_bad = -1, bad_rc = XMCA_OK;
  for (int64_t r = 0; r < world; ++r) {
    const int st_r = (int)all[((size_t)r * rows + cap) * width];
    if (st_r != XMCA_OK && first_bad < 0) { first_bad = (int)r; bad_rc = st_r; }
  }
  if (first_bad >= 0) {
    h->err = "rule_n_sharded: the shard of rank " + std::to_string(first_bad) + " failed with status " + std::to_string(bad_rc) +
             (local_rc != XMCA_OK ? " (this rank: " + local_err + ")" : " (this rank's shard was fine)");
    return local_rc != XMCA_OK ? local_rc : bad_rc;
  }
  for (int64_t r = 0; r < world; ++r) {
    const int64_t rb = begin_of(r), re = begin_of(r + 1);
    for (int64_t i = 0; i < re - rb; ++i) {
      const double* row = &all[((size_t)r * rows + i) * width];
      std::memcpy(spectra_out + (rb + i) * n_out, row, sizeof(double) * n_out);
      kept_out[rb + i] = (int)row[n_out];
    }
  }
  return XMCA_OK;
}

int xmca_rule_n_sharded(xmca_handle* h, xmca_comm* c, int64_t n_runs, int64_t T, int64_t Nx, int64_t Ny, int n_fields,
                        const double* hilbert_col, int rotated, int p, int power, double tol, uint64_t seed, int dtype,
                        double* spectra_out, int* kept_out, int64_t n_out) {
  return rule_n_sharded_body(h, c, n_runs, seed, spectra_out, kept_out, n_out, [&](int64_t b, int64_t e, uint64_t sd, double* sp, int* kp) {
    return xmca_rule_n(h, T, Nx, Ny, n_fields, hilbert_col, rotated, p, power, tol, b, e, sd, dtype, sp, kp, n_out);
  });
}

int xmca_rule_n_ar1_sharded(xmca_handle* h, xmca_comm* c, int64_t n_runs, int64_t T, int64_t Nx, int64_t Ny, int n_fields,
                            const double* hilbert_col, int rotated, int p, int power, double tol, uint64_t seed, int dtype,
                            double* spectra_out, int* kept_out, int64_t n_out, const double* phi_left, const double* phi_right) {
  return rule_n_sharded_body(h, c, n_runs, seed, spectra_out, kept_out, n_out, [&](int64_t b, int64_t e, uint64_t sd, double* sp, int* kp) {
    return xmca_rule_n_ar1(h, T, Nx, Ny, n_fields, hilbert_col, rotated, p, power, tol, b, e, sd, dtype, sp, kp, n_out, phi_left, phi_right);
  });
}

int xmca_surrogate(xmca_handle* h, int64_t n, uint64_t seed, uint32_t run, uint32_t side, double* out) {
  API_BEGIN(h)
  XMCA_CHECK(n >= 1 && out, XMCA_ERR_INVALID, "surrogate: bad arguments");
  DevBuf<double> d;
  hipLaunchKernelGGL((philox_normal_kernel<double>), ew_grid((n + 1) / 2), dim3(EW_BLOCK), 0, h->st, d.ensure((size_t)n), n, seed, run,
                     side);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(out, d.get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_get_reduction_info(xmca_handle* h, char* out, int out_len) {
  if (!h || !out || out_len < 1) return XMCA_ERR_INVALID;
  const std::string& d = h->ews.trd.last_desc;
  std::strncpy(out, d.c_str(), (size_t)out_len - 1);
  out[out_len - 1] = 0;
  return (int)d.size();
}

int xmca_get_timings(xmca_handle* h, char* names, int names_len, double* ms, int max_n) {
  if (!h) return XMCA_ERR_INVALID;
  try {                              // (the tail's time belongs to the step that queued it; its failure is the next reader's to report)
    if (h->tail.pending && h->tail.err_code == XMCA_OK) { (void)hipSetDevice(h->device); join_tail(h); }
    h->tm.collect();
  } catch (...) { return XMCA_ERR_HIP; }
  std::string joined;
  int n = 0;
  for (const auto& name : h->tm.order) {
    if (n >= max_n) break;
    if (n) joined += ";";
    joined += name;
    if (ms) ms[n] = h->tm.ms[name];
    ++n;
  }
  // kernel-level entries: total duration and launch count of the eigensolver's fused round kernel (hipEvents around the
  // rounds of every sweep, jacobi.h) - ms[] carries the count for the second name
  const double rk_ms = h->ews.round_ms;
  const double rk_n = (double)h->ews.round_launches;
  if (rk_n > 0 && n + 2 <= max_n) {
    joined += (n ? ";" : "") + std::string("jacobi_round_kernel_ms;jacobi_round_kernel_launches");
    if (ms) { ms[n] = rk_ms; ms[n + 1] = rk_n; }
    n += 2;
  }
  // ... and of the tridiagonal reduction (tridiag.h): total duration of the reduction kernel(s) and number of reductions
  if (h->ews.trd.reduce_calls > 0 && n + 3 <= max_n) {
    joined += (n ? ";" : "") + std::string("trd_reduce_kernel_ms;trd_reduce_calls;trd_resident_calls");
    if (ms) { ms[n] = h->ews.trd.reduce_ms; ms[n + 1] = (double)h->ews.trd.reduce_calls; ms[n + 2] = (double)h->ews.trd.resident_calls; }
    n += 3;
  }
  if (names && names_len > 0) {
    std::strncpy(names, joined.c_str(), (size_t)names_len - 1);
    names[names_len - 1] = 0;
  }
  return n;
}

int xmca_reset_timings(xmca_handle* h) {
  if (!h) return XMCA_ERR_INVALID;
  try {
    if (h->tail.pending && h->tail.err_code == XMCA_OK) { (void)hipSetDevice(h->device); join_tail(h); }
    h->tm.reset();
  } catch (...) { return XMCA_ERR_HIP; }
  h->ews.round_ms = 0.0;
  h->ews.round_launches = 0;
  h->ews.trd.reduce_ms = 0.0;
  h->ews.trd.reduce_calls = 0;
  h->ews.trd.resident_calls = 0;
  return XMCA_OK;
}

int xmca_fft(xmca_handle* h, const double* in_re, const double* in_im, int batch, int n, int sign, double* out_re, double* out_im) {
  API_BEGIN(h)
  XMCA_CHECK(in_re && out_re && out_im && batch >= 1 && n >= 2 && (sign == 1 || sign == -1), XMCA_ERR_INVALID, "fft: bad arguments");
  FftPlan plan;
  XMCA_CHECK(fft_plan(n, plan), XMCA_ERR_UNSUPPORTED, "fft: length must factor into 2, 3, 5, 7 and be at most 5120");
  const size_t cnt = (size_t)batch * n;
  DevBuf<double> ir, ii, orr, oi;
  XMCA_HIP(hipMemcpyAsync(ir.ensure(cnt), in_re, sizeof(double) * cnt, hipMemcpyHostToDevice, h->st));
  if (in_im) XMCA_HIP(hipMemcpyAsync(ii.ensure(cnt), in_im, sizeof(double) * cnt, hipMemcpyHostToDevice, h->st));
  fft_batch(h->st, plan, batch, ir.get(), in_im ? ii.get() : nullptr, n, 1, (double)sign, orr.ensure(cnt), oi.ensure(cnt), n, 1, n, nullptr,
            nullptr, 1.0);
  XMCA_HIP(hipMemcpyAsync(out_re, orr.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(out_im, oi.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_pool_bytes(xmca_handle* h, int64_t* held_bytes) {
  if (!h || !held_bytes) return XMCA_ERR_INVALID;
  size_t total = 0;
  { std::lock_guard<std::mutex> g(h->pool.mu); total += h->pool.held; }
  for (xmca_handle* lane : h->lanes) { std::lock_guard<std::mutex> g(lane->pool.mu); total += lane->pool.held; }
  *held_bytes = (int64_t)total;
  return XMCA_OK;
}

int xmca_trim_pool(xmca_handle* h) {
  API_BEGIN(h)
  XMCA_HIP(hipStreamSynchronize(h->st));
  h->pool.trim();
  h->tail.trim();                    // (joined above: split-K slabs and partial sums of the deferred back-projection)
  for (xmca_handle* lane : h->lanes) {
    XMCA_HIP(hipStreamSynchronize(lane->st));
    lane->pool.trim();
  }
  API_END(h)
}

int xmca_gemm(xmca_handle* h, const void* A, int64_t lda, int a_kfast, const void* B, int64_t ldb, int b_nfast, double* C, int M,
              int N, int K, int dtype, double alpha, int upper_only, int mirror, int splits) {
  API_BEGIN(h)
  XMCA_CHECK(A && B && C && M > 0 && N > 0 && K >= 0, XMCA_ERR_INVALID, "gemm: bad arguments");
  const size_t na = (size_t)(a_kfast ? M : K) * lda, nb = (size_t)(b_nfast ? K : N) * ldb;
  GemmOpts o;
  o.a_kfast = a_kfast != 0; o.b_nfast = b_nfast != 0; o.alpha = alpha; o.upper_only = upper_only != 0; o.mirror = mirror;
  o.force_splits = splits;
  with_dtype(dtype, [&](auto t) {
    using TI = decltype(t);
    DevBuf<TI> Ad, Bd;
    DevBuf<double> Cd;
    XMCA_HIP(hipMemcpyAsync(Ad.ensure(na), A, na * sizeof(TI), hipMemcpyHostToDevice, h->st));
    XMCA_HIP(hipMemcpyAsync(Bd.ensure(nb), B, nb * sizeof(TI), hipMemcpyHostToDevice, h->st));
    Cd.ensure((size_t)M * N);
    XMCA_HIP(hipMemsetAsync(Cd.get(), 0, sizeof(double) * (size_t)M * N, h->st));
    gemm<TI, double>(h->st, h->gws, Ad.get(), lda, Bd.get(), ldb, Cd.get(), N, M, N, K, o);
    XMCA_HIP(hipMemcpyAsync(C, Cd.get(), sizeof(double) * (size_t)M * N, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
  });
  API_END(h)
}

int xmca_gemm_ex(xmca_handle* h, const void* A, int64_t lda, int a_kfast, const void* B, int64_t ldb, int b_nfast, void* C,
                 int64_t ldc, int c_dtype, int M, int N, int K, int dtype, double alpha, double beta, const double* row_scale,
                 const double* col_scale, int upper_only, int mirror, int splits) {
  API_BEGIN(h)
  XMCA_CHECK(A && B && C && M > 0 && N > 0 && K >= 0 && ldc >= N, XMCA_ERR_INVALID, "gemm_ex: bad arguments");
  XMCA_CHECK(lda >= (a_kfast ? K : M) && ldb >= (b_nfast ? N : K), XMCA_ERR_INVALID, "gemm_ex: leading dimension below the extent");
  const size_t na = (size_t)(a_kfast ? M : K) * lda, nb = (size_t)(b_nfast ? K : N) * ldb, nc = (size_t)M * ldc;
  DevBuf<double> rs, cs;
  GemmOpts o;
  o.a_kfast = a_kfast != 0; o.b_nfast = b_nfast != 0; o.alpha = alpha; o.beta = beta; o.upper_only = upper_only != 0; o.mirror = mirror;
  o.force_splits = splits;
  if (row_scale) {
    XMCA_HIP(hipMemcpyAsync(rs.ensure(M), row_scale, sizeof(double) * M, hipMemcpyHostToDevice, h->st));
    o.row_scale = rs.get();
  }
  if (col_scale) {
    XMCA_HIP(hipMemcpyAsync(cs.ensure(N), col_scale, sizeof(double) * N, hipMemcpyHostToDevice, h->st));
    o.col_scale = cs.get();
  }
  with_dtype(dtype, [&](auto ti) {
    using TI = decltype(ti);
    with_dtype(c_dtype, [&](auto to) {
      using TO = decltype(to);
      DevBuf<TI> Ad, Bd;
      DevBuf<TO> Cd;
      XMCA_HIP(hipMemcpyAsync(Ad.ensure(na), A, na * sizeof(TI), hipMemcpyHostToDevice, h->st));
      XMCA_HIP(hipMemcpyAsync(Bd.ensure(nb), B, nb * sizeof(TI), hipMemcpyHostToDevice, h->st));
      // C goes up whatever beta is: the padding of its rows and, with beta = 0, what it held before must come back as they were / unread
      XMCA_HIP(hipMemcpyAsync(Cd.ensure(nc), C, nc * sizeof(TO), hipMemcpyHostToDevice, h->st));
      gemm<TI, TO>(h->st, h->gws, Ad.get(), lda, Bd.get(), ldb, Cd.get(), ldc, M, N, K, o);
      XMCA_HIP(hipMemcpyAsync(C, Cd.get(), nc * sizeof(TO), hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipStreamSynchronize(h->st));
    });
  });
  API_END(h)
}

int xmca_cholesky(xmca_handle* h, const double* A, int n, int is_complex, double rel_shift, double* R, int* ok) {
  API_BEGIN(h)
  XMCA_CHECK(A && R && ok && n >= 1, XMCA_ERR_INVALID, "cholesky: bad arguments");
  const bool cplx = is_complex != 0;
  const size_t nn = (size_t)n * n;
  DevBuf<double> raw, rout;
  CPlanes Ap;
  Ap.ensure(nn, cplx);
  if (cplx) {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(2 * nn), A, sizeof(double) * 2 * nn, hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL((split_complex_kernel<double, double>), ew_grid((int64_t)nn), dim3(EW_BLOCK), 0, h->st, raw.get(), Ap.r(),
                       Ap.im.get(), (int64_t)nn);
  } else {
    XMCA_HIP(hipMemcpyAsync(Ap.r(), A, sizeof(double) * nn, hipMemcpyHostToDevice, h->st));
  }
  *ok = cholesky_upper(h->st, h->gws, Ap.r(), Ap.i(cplx), n, n, rel_shift) ? 1 : 0;
  const size_t no = nn * (cplx ? 2 : 1);
  hipLaunchKernelGGL((pack_rows_kernel<double>), ew_grid((int64_t)nn), dim3(EW_BLOCK), 0, h->st, Ap.r(), Ap.i(cplx), (int64_t)n, n, n,
                     rout.ensure(no), 0);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(R, rout.get(), sizeof(double) * no, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_cholesky_ex(xmca_handle* h, const double* A, int n, int64_t lda, int first, int is_complex, double rel_shift, double* R, int* ok) {
  API_BEGIN(h)
  XMCA_CHECK(A && R && ok && n >= 1 && lda >= n && first >= 0 && first < n, XMCA_ERR_INVALID, "cholesky_ex: bad arguments");
  const bool cplx = is_complex != 0;
  const size_t cnt = (size_t)n * (size_t)lda, no = cnt * (cplx ? 2 : 1);
  DevBuf<double> raw, rout;
  CPlanes Ap;
  Ap.ensure(cnt, cplx);
  if (cplx) {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(2 * cnt), A, sizeof(double) * 2 * cnt, hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL((split_complex_kernel<double, double>), ew_grid((int64_t)cnt), dim3(EW_BLOCK), 0, h->st, raw.get(), Ap.r(),
                       Ap.im.get(), (int64_t)cnt);
  } else {
    XMCA_HIP(hipMemcpyAsync(Ap.r(), A, sizeof(double) * cnt, hipMemcpyHostToDevice, h->st));
  }
  // the trailing block behind row / column `first`, the way factor_by_cholesky (solver.h) poses it: base + first * (lda + 1), ld = lda
  const size_t off = (size_t)first * (size_t)(lda + 1);
  *ok = cholesky_upper(h->st, h->gws, Ap.r() + off, cplx ? Ap.im.get() + off : nullptr, n - first, lda, rel_shift) ? 1 : 0;
  hipLaunchKernelGGL((pack_rows_kernel<double>), ew_grid((int64_t)cnt), dim3(EW_BLOCK), 0, h->st, Ap.r(), Ap.i(cplx), lda, n, (int)lda,
                     rout.ensure(no), 0);
  XMCA_HIP(hipGetLastError());
  XMCA_HIP(hipMemcpyAsync(R, rout.get(), sizeof(double) * no, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

int xmca_lead_rows(xmca_handle* h, const double* A, int64_t lda, const double* B, int64_t ldb, int b_kfast, int rows, int K, int n,
                   const double* scale, double* out, int64_t ldo, int* chunks) {
  API_BEGIN(h)
  XMCA_CHECK(A && B && out && rows >= 1 && rows <= LEAD_ROWS && K >= 1 && n >= 1 && lda >= K && ldo >= n && ldb >= (b_kfast ? K : n),
             XMCA_ERR_INVALID, "lead_rows: bad arguments");
  const size_t na = (size_t)rows * (size_t)lda, nb = (size_t)(b_kfast ? n : K) * (size_t)ldb, no = (size_t)rows * (size_t)ldo;
  DevBuf<double> Ad, Bd, Sd, Od, part;
  XMCA_HIP(hipMemcpyAsync(Ad.ensure(na), A, sizeof(double) * na, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Bd.ensure(nb), B, sizeof(double) * nb, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(Od.ensure(no), out, sizeof(double) * no, hipMemcpyHostToDevice, h->st));
  if (scale) XMCA_HIP(hipMemcpyAsync(Sd.ensure((size_t)rows), scale, sizeof(double) * rows, hipMemcpyHostToDevice, h->st));
  lead_rows(h->st, b_kfast != 0, Ad.get(), lda, Bd.get(), ldb, rows, K, n, Od.get(), ldo, scale ? Sd.get() : nullptr, part);
  XMCA_HIP(hipMemcpyAsync(out, Od.get(), sizeof(double) * no, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  if (chunks) *chunks = ceil_div(K, lead_rows_chunk(K, n));
  API_END(h)
}

int xmca_fft_ex(xmca_handle* h, const double* in_re, const double* in_im, int64_t in_count, int64_t in_bs, int64_t in_es, int n_in,
                int conj_in, const double* sin_, int batch, int n, int sign, double* out_re, double* out_im, int64_t out_count,
                int64_t out_bs, int64_t out_es, int n_keep, const double* sa, const double* sb, double scale) {
  API_BEGIN(h)
  XMCA_CHECK(in_re && out_re && out_im && batch >= 1 && n >= 2 && (sign == 1 || sign == -1) && in_count >= 1 && out_count >= 1,
             XMCA_ERR_INVALID, "fft_ex: bad arguments");
  XMCA_CHECK(n_in >= 1 && n_in <= n && n_keep >= 1 && n_keep <= n, XMCA_ERR_INVALID, "fft_ex: n_in and n_keep lie in [1, n]");
  // an index b * bs + t * es is linear in (b, t): its extremes are at the corners of [0, batch) x [0, count)
  auto inside = [&](int64_t bs, int64_t es, int len, int64_t count) {
    const int64_t lim = (int64_t)1 << 30;      // (products with a 31-bit index stay inside int64)
    if (bs <= -lim || bs >= lim || es <= -lim || es >= lim) return false;
    for (int64_t b : {(int64_t)0, (int64_t)batch - 1})
      for (int64_t t : {(int64_t)0, (int64_t)len - 1}) {
        const int64_t i = b * bs + t * es;
        if (i < 0 || i >= count) return false;
      }
    return true;
  };
  XMCA_CHECK(inside(in_bs, in_es, n_in, in_count), XMCA_ERR_INVALID, "fft_ex: an input index lies outside the input");
  XMCA_CHECK(inside(out_bs, out_es, n_keep, out_count), XMCA_ERR_INVALID, "fft_ex: an output index lies outside the output");
  FftPlan plan;
  XMCA_CHECK(fft_plan(n, plan), XMCA_ERR_UNSUPPORTED, "fft_ex: length must factor into 2, 3, 5, 7 and be at most 5120");
  const size_t ni = (size_t)in_count, nout = (size_t)out_count;
  DevBuf<double> ir, ii, orr, oi, fs, fa, fb;
  XMCA_HIP(hipMemcpyAsync(ir.ensure(ni), in_re, sizeof(double) * ni, hipMemcpyHostToDevice, h->st));
  if (in_im) XMCA_HIP(hipMemcpyAsync(ii.ensure(ni), in_im, sizeof(double) * ni, hipMemcpyHostToDevice, h->st));
  if (sin_) XMCA_HIP(hipMemcpyAsync(fs.ensure((size_t)n_in), sin_, sizeof(double) * n_in, hipMemcpyHostToDevice, h->st));
  if (sa) XMCA_HIP(hipMemcpyAsync(fa.ensure((size_t)n_keep), sa, sizeof(double) * n_keep, hipMemcpyHostToDevice, h->st));
  if (sb) XMCA_HIP(hipMemcpyAsync(fb.ensure((size_t)batch), sb, sizeof(double) * batch, hipMemcpyHostToDevice, h->st));
  // the outputs go up first: what the kernel must not touch comes back as it went in
  XMCA_HIP(hipMemcpyAsync(orr.ensure(nout), out_re, sizeof(double) * nout, hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(oi.ensure(nout), out_im, sizeof(double) * nout, hipMemcpyHostToDevice, h->st));
  fft_batch(h->st, plan, batch, ir.get(), in_im ? ii.get() : nullptr, in_bs, in_es, (double)sign, orr.get(), oi.get(), out_bs, out_es, n_keep,
            sa ? fa.get() : nullptr, sb ? fb.get() : nullptr, scale, n_in, conj_in != 0, sin_ ? fs.get() : nullptr);
  XMCA_HIP(hipMemcpyAsync(out_re, orr.get(), sizeof(double) * nout, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipMemcpyAsync(out_im, oi.get(), sizeof(double) * nout, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

// xmca_tridiag_eigenvalues and xmca_tridiag_vectors: (d, e) (and `extra`, n_extra values in the same scale) times the power of two
// a solve would apply - trd_scale_kernel itself decides it, from max(|d|, |e|) as the bit pattern trd_maxabs_kernel leaves behind -
// into dd / de / dx.  ws.scal and ws.flag are left as trd_reduce leaves them.  Returns false (nothing scaled: f = 1, scal[1] = 1)
// when an entry is not finite.  Synchronises the stream.
static bool tridiag_stage_upload(xmca_handle* h, TrdWorkspace& ws, const double* d, const double* e, int n, const double* extra, int n_extra,
                                 DevBuf<double>& dd, DevBuf<double>& de, DevBuf<double>& dx) {
  double m = 0.0;
  bool bad = false;
  auto see = [&](double v) {
    const double a = std::fabs(v);
    if (!(a <= 1.7e308)) bad = true;
    else if (a > m) m = a;
  };
  for (int i = 0; i < n; ++i) see(d[i]);
  for (int i = 0; i + 1 < n; ++i) see(e[i]);
  for (int i = 0; i < n_extra; ++i)
    if (!(std::fabs(extra[i]) <= 1.7e308)) bad = true;
  unsigned long long acc[2] = {0ull, bad ? 1ull : 0ull};
  if (!bad) std::memcpy(&acc[0], &m, sizeof(double));
  ws.scal.ensure(4);
  ws.flag.ensure(4);
  XMCA_HIP(hipMemsetAsync(ws.flag.get(), 0, sizeof(int) * 4, h->st));
  unsigned long long* dacc = reinterpret_cast<unsigned long long*>(ws.scal.get() + 2);
  XMCA_HIP(hipMemcpyAsync(dacc, acc, sizeof(acc), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(trd_scale_kernel, dim3(1), dim3(1), 0, h->st, dacc, ws.scal.get());
  XMCA_HIP(hipGetLastError());
  double scal[2] = {1.0, 0.0};
  XMCA_HIP(hipMemcpyAsync(scal, ws.scal.get(), sizeof(scal), hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  const double f = scal[0];                      // (a power of two: the products below are the ones trd_copy_kernel forms)
  std::vector<double> hd((size_t)n), he((size_t)std::max(n - 1, 1), 0.0), hx((size_t)std::max(n_extra, 1), 0.0);
  for (int i = 0; i < n; ++i) hd[i] = f * d[i];
  for (int i = 0; i + 1 < n; ++i) he[i] = f * e[i];
  for (int i = 0; i < n_extra; ++i) hx[i] = f * extra[i];
  XMCA_HIP(hipMemcpyAsync(dd.ensure(hd.size()), hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(de.ensure(he.size()), he.data(), sizeof(double) * he.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipMemcpyAsync(dx.ensure(hx.size()), hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));         // (the host copies go out of scope)
  return !bad;
}

int xmca_tridiag_eigenvalues(xmca_handle* h, const double* d, const double* e, int n, double* lam_desc) {
  if (!d || !lam_desc || n < 1 || (!e && n > 1)) return XMCA_ERR_INVALID;
  API_BEGIN(h)
  XMCA_CHECK((size_t)n * 16 <= (size_t)150 * 1024, XMCA_ERR_UNSUPPORTED, "tridiag_eigenvalues: the matrix does not fit the LDS of a workgroup");
  TrdWorkspace ws;
  DevBuf<double> dd, de, dx, lam_tmp;
  tridiag_stage_upload(h, ws, d, e, n, nullptr, 0, dd, de, dx);
  TrdParams P{};
  P.n = n;
  P.d = dd.get();
  P.e = de.get();
  std::vector<double> lam;
  trd_eigenvalues(h->st, ws, P, lam, nullptr, lam_tmp);       // (a non-finite entry: the numeric error of a solve)
  std::memcpy(lam_desc, lam.data(), sizeof(double) * (size_t)n);
  API_END(h)
}

int xmca_tridiag_vectors(xmca_handle* h, const double* d, const double* e, int n, const double* lam, int nev, double* Y, int64_t ldy) {
  if (!d || !lam || !Y || n < 1 || (!e && n > 1) || nev < 1 || nev > n || ldy < nev) return XMCA_ERR_INVALID;
  API_BEGIN(h)
  TrdWorkspace ws;
  DevBuf<double> dd, de, dl, W, Yd;
  TrdTwistScratch twist;
  const bool finite = tridiag_stage_upload(h, ws, d, e, n, lam, nev, dd, de, dl);
  XMCA_CHECK(finite, XMCA_ERR_NUMERIC, "tridiag_vectors: d, e and lam must be finite");
  const size_t plane = (size_t)n * (size_t)ldy;
  W.ensure(plane);
  XMCA_HIP(hipMemcpyAsync(Yd.ensure(plane), Y, sizeof(double) * plane, hipMemcpyHostToDevice, h->st));
  trd_twisted_vectors(h->st, dd.get(), de.get(), n, nev, dl.get(), W.get(), Yd.get(), ldy, twist);
  XMCA_HIP(hipMemcpyAsync(Y, Yd.get(), sizeof(double) * plane, hipMemcpyDeviceToHost, h->st));
  XMCA_HIP(hipStreamSynchronize(h->st));
  API_END(h)
}

// xmca_eigh and xmca_eigh_lead: upload, hermitian_evd, packed rows back.  n_lead < 0: the n x n planes of xmca_eigh.  Otherwise the
// planes handed to hermitian_evd have n_lead + 1 rows of ldz = (n rounded up to 16) + 16 elements, the padding columns and the
// extra row filled with a sentinel beforehand; *guard_clean says whether every sentinel word is still there afterwards.
static void eigh_body(xmca_handle* h, const double* A, int n, bool cplx, int n_lead, double* lam, double* Zh, EvdInfo& ei, int* guard_clean) {
  const size_t nn = (size_t)n * n;
  const bool lead = n_lead >= 0;
  const int rows = lead ? n_lead : n;
  const int64_t ldz = lead ? (((int64_t)n + 15) & ~(int64_t)15) + 16 : n;
  const size_t zcount = lead ? (size_t)(rows + 1) * (size_t)ldz : nn;
  DevBuf<double> raw, zout;
  CPlanes Ap, Zp;
  Ap.ensure(nn, cplx);
  Zp.ensure(zcount, cplx);
  if (cplx) {
    XMCA_HIP(hipMemcpyAsync(raw.ensure(2 * nn), A, sizeof(double) * 2 * nn, hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL((split_complex_kernel<double, double>), ew_grid((int64_t)nn), dim3(EW_BLOCK), 0, h->st, raw.get(), Ap.r(),
                       Ap.im.get(), (int64_t)nn);
  } else {
    XMCA_HIP(hipMemcpyAsync(Ap.r(), A, sizeof(double) * nn, hipMemcpyHostToDevice, h->st));
  }
  const uint64_t sentinel_bits = 0xC7D5A5A5A5A5A5A5ull;       // (a finite double nobody computes)
  double sentinel;
  std::memcpy(&sentinel, &sentinel_bits, sizeof(sentinel));
  std::vector<double> guard;
  if (lead) {
    guard.assign(zcount, sentinel);
    for (int c = 0; c < (cplx ? 2 : 1); ++c)
      XMCA_HIP(hipMemcpyAsync(c ? Zp.im.get() : Zp.r(), guard.data(), sizeof(double) * zcount, hipMemcpyHostToDevice, h->st));
  }
  std::vector<double> lh;
  XMCA_HIP(hipStreamSynchronize(h->st));
  h->tm.begin(Zh ? "eigh_vectors" : "eigh_values");
  // Zh == NULL: eigenvalues only (the n_vec = 0 solves of rule_n; tridiagonal route of csrc/tridiag.h)
  hermitian_evd(h->st, h->ews, Ap.r(), Ap.i(cplx), n, n, lh, nullptr, Zh ? Zp.r() : nullptr, Zh ? Zp.i(cplx) : nullptr, ldz, &ei, false,
                lead ? n_lead : -1);
  h->tm.end();
  std::memcpy(lam, lh.data(), sizeof(double) * n);
  if (Zh) {
    const size_t cnt = (size_t)rows * n, no = cnt * (cplx ? 2 : 1);
    hipLaunchKernelGGL((pack_rows_kernel<double>), ew_grid((int64_t)cnt), dim3(EW_BLOCK), 0, h->st, Zp.r(), Zp.i(cplx), ldz, rows, n,
                       zout.ensure(no), 0);
    XMCA_HIP(hipGetLastError());
    XMCA_HIP(hipMemcpyAsync(Zh, zout.get(), sizeof(double) * no, hipMemcpyDeviceToHost, h->st));
    XMCA_HIP(hipStreamSynchronize(h->st));
  }
  if (lead) {
    bool clean = true;
    for (int c = 0; c < (cplx ? 2 : 1); ++c) {
      XMCA_HIP(hipMemcpyAsync(guard.data(), c ? Zp.im.get() : Zp.r(), sizeof(double) * zcount, hipMemcpyDeviceToHost, h->st));
      XMCA_HIP(hipStreamSynchronize(h->st));
      for (int r = 0; r <= rows && clean; ++r)
        for (int64_t q = r < rows ? n : 0; q < ldz && clean; ++q)
          clean = std::memcmp(&guard[(size_t)r * (size_t)ldz + (size_t)q], &sentinel, sizeof(double)) == 0;
    }
    *guard_clean = clean ? 1 : 0;
  }
}

int xmca_eigh(xmca_handle* h, const double* A, int n, int is_complex, double* lam, double* Zh, int* info) {
  API_BEGIN(h)
  XMCA_CHECK(A && n >= 1 && lam, XMCA_ERR_INVALID, "eigh: bad arguments");
  EvdInfo ei;
  eigh_body(h, A, n, is_complex != 0, -1, lam, Zh, ei, nullptr);
  if (info) { info[0] = ei.sweeps; info[1] = ei.tile; info[2] = ei.slots; info[3] = ei.lr_step + 2 * ei.tridiag; }
  API_END(h)
}

int xmca_eigh_lead(xmca_handle* h, const double* A, int n, int is_complex, int n_lead, double* lam, double* Zh, int* info) {
  API_BEGIN(h)
  XMCA_CHECK(A && n >= 1 && lam && Zh && info && n_lead >= 1 && n_lead <= n, XMCA_ERR_INVALID, "eigh_lead: bad arguments");
  EvdInfo ei;
  int clean = 0;
  eigh_body(h, A, n, is_complex != 0, n_lead, lam, Zh, ei, &clean);
  info[0] = ei.sweeps; info[1] = ei.tile; info[2] = ei.slots; info[3] = ei.lr_step + 2 * ei.tridiag; info[4] = ei.n_eigvec; info[5] = clean;
  API_END(h)
}

int xmca_partial_count(const double* lam_desc, int n, int n_lead, int* rep_lead) {
  if (!lam_desc || n < 1) return -1;
  const std::vector<double> lam(lam_desc, lam_desc + n);
  const int kp = trd_partial_count(lam, n, n_lead);
  if (rep_lead) *rep_lead = trd_repeated_leading(lam, n, kp) ? 1 : 0;
  return kp;
}

int xmca_bench_gram(xmca_handle* h, int side, int reps, double* avg_ms, double* kernel_ms, double* flops) {
  API_BEGIN(h)
  XMCA_CHECK((side == 0 || side == 1) && h->field_set[side] && reps >= 1, XMCA_ERR_STATE, "bench_gram: field not set");
  int64_t T = 0, N = 0;
  with_dtype(h->dtype, [&](auto t) { T = typed<decltype(t)>(h).f[side].T; N = typed<decltype(t)>(h).f[side].N; });
  DevBuf<double> G;
  G.ensure((size_t)T * T);
  std::vector<hipEvent_t> ev(2 * (size_t)reps + 2);
  for (auto& e : ev) XMCA_HIP(hipEventCreate(&e));
  auto run = [&](hipEvent_t b, hipEvent_t e) {
    GemmOpts o;
    o.b_nfast = false; o.upper_only = true; o.mirror = 1; o.ev_begin = b; o.ev_end = e;
    with_dtype(h->dtype, [&](auto t) {
      using TI = decltype(t);
      const TI* x = typed<TI>(h).f[side].r();
      gemm<TI, double>(h->st, h->gws, x, N, x, N, G.get(), T, (int)T, (int)T, (int)N, o);
    });
  };
  run(nullptr, nullptr);   // warm-up
  XMCA_HIP(hipStreamSynchronize(h->st));
  XMCA_HIP(hipEventRecord(ev[2 * reps], h->st));
  for (int i = 0; i < reps; ++i) run(ev[2 * i], ev[2 * i + 1]);
  XMCA_HIP(hipEventRecord(ev[2 * reps + 1], h->st));
  XMCA_HIP(hipEventSynchronize(ev[2 * reps + 1]));
  float ms = 0.f;
  XMCA_HIP(hipEventElapsedTime(&ms, ev[2 * reps], ev[2 * reps + 1]));
  double kms = 0.0;
  for (int i = 0; i < reps; ++i) {
    float t = 0.f;
    XMCA_HIP(hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
    kms += t;
  }
  if (avg_ms) *avg_ms = ms / reps;
  if (kernel_ms) *kernel_ms = kms / reps;
  if (flops) *flops = (double)T * (double)(T + 1) * (double)N;
  for (auto& e : ev) (void)hipEventDestroy(e);
  API_END(h)
}

int xmca_bench_gemm(xmca_handle* h, int M, int N, int K, int dtype, int a_kfast, int b_nfast, int upper_only, int splits,
                    int reps, double* avg_ms) {
  API_BEGIN(h)
  XMCA_CHECK(M > 0 && N > 0 && K > 0 && reps > 0 && avg_ms, XMCA_ERR_INVALID, "bench_gemm: bad arguments");
  with_dtype(dtype, [&](auto t) { bench_gemm_impl<decltype(t)>(h, M, N, K, a_kfast, b_nfast, upper_only, splits, reps, avg_ms); });
  API_END(h)
}

}  // extern "C"
