// extern "C" surface of libccgp (include/ccgp.h).  Host orchestration only: argument
// checks, device scratch, chunking of batches, and the handful of host-side scalars
// (log-Jacobian, log-prior, quadrature nodes) that the reference computes in R.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <map>
#include <memory>
#include <new>
#include <vector>

#include "call_stage.h"
#include "ccgp_internal.h"
#include "chain_terms.h"
#include "cgp_fit_logic.h"
#include "fit_logic.h"
#include "nm_logic.h"
#include "special_math.h"

using namespace ccgp;

namespace {

#define CCGP_HIP(call)                                                              \
  do {                                                                              \
    hipError_t e_ = (call);                                                         \
    if (e_ != hipSuccess) {                                                         \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
      return CCGP_EHIP;                                                             \
    }                                                                               \
  } while (0)

int fail(ccgp_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// for the catch handlers: assigning the message may itself throw when memory is gone
int fail_noexcept(ccgp_handle* h, int code, const char* msg) noexcept {
  try {
    if (h) h->err = msg;
  } catch (...) {
  }
  return code;
}

// after enqueueing kernels: launch errors, and a refused kernel-attribute request (raise_lds_limit)
#define CCGP_LAUNCH_CHECK()                                                         \
  do {                                                                              \
    CCGP_HIP(hipGetLastError());                                                    \
    {                                                                               \
      const std::string ae_ = ccgp::attr_error(h->device);                          \
      if (!ae_.empty()) return fail(h, CCGP_EHIP, ae_);                             \
    }                                                                               \
  } while (0)

// the B draws at `params` as the kernels see them, in kernel family `fam`; refuses what that family cannot do (the
// Matern / spline families exist for the 1-D scripts only).  Callers run this BEFORE they push their inputs: a refused
// call costs no PCIe traffic.
int draw_view(ccgp_handle* h, const KernelFamily& fam, const double* params, int B, int K, int d, DrawView* dv) {
  *dv = DrawView{params, B, K, d, fam};
  if (fam.id != 0 && d != 1)
    return fail(h, CCGP_EUNSUPPORTED, "the Matern / spline families are one-dimensional (D1:348-389): d must be 1");
  if (fam.id == 2 && K != 2)
    return fail(h, CCGP_EUNSUPPORTED, "CCGP_KERNEL_MATERN_SPLINE is the two-family script's pair (D1F:453-462): K must be 2");
  return CCGP_OK;
}

// the scheduler's time account (ccgp_last_sched_profile) lies inside the memory of the sweep that wrote it: whoever frees
// [mem, mem + bytes) forgets the account with it
void forget_sched_profile(ccgp_handle* h, const void* mem, size_t bytes) {
  const char *p = reinterpret_cast<const char*>(h->sched_prof_dev), *m = static_cast<const char*>(mem);
  if (!p || p < m || p >= m + bytes) return;
  h->sched_prof_dev = nullptr;
  h->sched_prof_wgs = 0;
}

// The handle's three buffers -- device workspace, device staging, pinned host buffer of the copy path -- are grow-only:
// a request beyond the size frees (after the stream has drained) and allocates anew, `slack` adding 25 % + 4096 B so
// that a slowly growing series of calls does not reallocate each time.  `what` opens the error text.
struct BufferKind {
  hipError_t (*alloc)(void**, size_t);
  hipError_t (*release)(void*);
  bool slack;
  bool host;   // host memory: ccgp_debug_fill_scratch fills it with memset
  const char* what;
};
const BufferKind kWorkspace{[](void** p, size_t n) { return hipMalloc(p, n); }, [](void* p) { return hipFree(p); }, false,
                            false, "device workspace allocation"};
const BufferKind kStaging{kWorkspace.alloc, kWorkspace.release, true, false, "device staging allocation"};
const BufferKind kPinned{[](void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); },
                         [](void* p) { return hipHostFree(p); }, true, true, "pinned host buffer"};

// ccgp_debug_fill_scratch: [p, p + bytes) starts as `byte` repeated.  Device memory on the handle's stream, where every
// user of the memory is ordered behind it; host memory once that stream has drained.
int debug_fill(ccgp_handle* h, void* p, size_t bytes, bool host, int byte) {
  if (!p || !bytes) return CCGP_OK;
  if (!host) {
    CCGP_HIP(hipMemsetAsync(p, byte, bytes, h->stream));
    return CCGP_OK;
  }
  CCGP_HIP(hipStreamSynchronize(h->stream));
  std::memset(p, byte, bytes);
  return CCGP_OK;
}

int ensure(ccgp_handle* h, Buffer& b, const BufferKind& k, size_t bytes) {
  if (bytes <= b.bytes) return CCGP_OK;
  if (b.ptr) {
    CCGP_HIP(hipStreamSynchronize(h->stream));
    forget_sched_profile(h, b.ptr, b.bytes);
    CCGP_HIP(k.release(b.ptr));
    b = Buffer{};
  }
  const size_t want = k.slack ? bytes + bytes / 4 + 4096 : bytes;
  if (k.alloc(&b.ptr, want) != hipSuccess) {
    b.ptr = nullptr;
    return fail(h, CCGP_ENOMEM, std::string(k.what) + " of " + std::to_string(want) + " B failed");
  }
  b.bytes = want;
  if (h->debug_fill >= 0) return debug_fill(h, b.ptr, b.bytes, k.host, h->debug_fill);
  return CCGP_OK;
}

// the staging buffer of one call: `lay` declares its pieces (stage_layout.h) and runs twice, once to size the buffer and
// once, over the buffer, to hand out the pointers
template <class F>
int stage(ccgp_handle* h, F&& lay) {
  if (int rc = ensure(h, h->stage, kStaging, layout_bytes(lay))) return rc;
  Layout real(h->stage.ptr);
  lay(real);
  return CCGP_OK;
}

// ---- host <-> device traffic of the host-pointer entry points ------------------------------------------------
// The pieces of a call lie back to back in the handle's staging buffer (Layout).  A hipMemcpyAsync from / to
// pageable memory is a staged, synchronous copy of its own (10 - 20 us each); what the reference's callers issue
// are many SMALL calls (predict.post per draw and test site HX:688, beta.MLE / factors per draw HX:641), so up to
// kPinMax the host image of the whole span is assembled in the handle's pinned buffer and crosses PCIe in ONE copy
// each way; larger payloads are copied piece by piece as before.  pin_max lowers that bound for a call that has
// measured a smaller one (ccgp_loglik_batch); 0 means piece by piece.
constexpr size_t kPinMax = size_t(8) << 20;
constexpr int kPullSlices = ccgp::kPullSlices;

int push(ccgp_handle* h, Pieces ps, size_t pin_max = kPinMax) {
  const Span sp = span_of(ps);
  char* const lo = sp.lo;
  const size_t span = sp.bytes;
  h->pin_in = 0;
  if (!lo) return CCGP_OK;
  if (span <= pin_max && ensure(h, h->pin, kPinned, span) == CCGP_OK) {
    char* pin = static_cast<char*>(h->pin.ptr);
    for (const Piece& p : ps)
      if (p.host && p.bytes) std::memcpy(pin + (static_cast<char*>(p.dev) - lo), p.host, p.bytes);
    CCGP_HIP(hipMemcpyAsync(lo, pin, span, hipMemcpyHostToDevice, h->stream));
    h->pin_in = Layout::al(span);
    return CCGP_OK;
  }
  for (const Piece& p : ps)
    if (p.host && p.bytes) CCGP_HIP(hipMemcpyAsync(p.dev, p.host, p.bytes, hipMemcpyHostToDevice, h->stream));
  return CCGP_OK;
}

// device -> host of the result pieces, then the stream is synchronised (the call's results are valid on return)
int pull(ccgp_handle* h, Pieces ps, size_t pin_max = kPinMax) {
  const Span sp = span_of(ps);
  char* const lo = sp.lo;
  const size_t span = sp.bytes;
  if (!lo) {
    CCGP_HIP(hipStreamSynchronize(h->stream));
    return CCGP_OK;
  }
  if (span <= pin_max && ensure(h, h->pin, kPinned, h->pin_in + span) == CCGP_OK) {
    char* pin = static_cast<char*>(h->pin.ptr) + h->pin_in;
    // a large result (the S x m tables of ccgp_predict_batch: 2.4 MB per Ground-Vibrations set) comes back in four
    // slices, each followed by an event: the host copies slice c out of the pinned buffer while slice c + 1 is still
    // crossing PCIe, instead of waiting for all of it and then copying all of it
    const int nsl = span >= (size_t(512) << 10) ? kPullSlices : 1;
    if (nsl > 1 && !h->pull_ev[0]) {
      for (int c = 0; c < kPullSlices; ++c)
        if (hipEventCreateWithFlags(&h->pull_ev[c], hipEventDisableTiming) != hipSuccess) {
          for (int q = 0; q < c; ++q) (void)hipEventDestroy(h->pull_ev[q]);
          h->pull_ev[0] = nullptr;
          h->err = "hipEventCreateWithFlags failed";
          return CCGP_EHIP;
        }
    }
    const size_t step = ((span + nsl - 1) / nsl + 255) / 256 * 256;
    for (int c = 0; c < nsl; ++c) {
      const size_t a = std::min(span, (size_t)c * step), b = std::min(span, a + step);
      if (b > a) CCGP_HIP(hipMemcpyAsync(pin + a, lo + a, b - a, hipMemcpyDeviceToHost, h->stream));
      if (nsl > 1) CCGP_HIP(hipEventRecord(h->pull_ev[c], h->stream));
    }
    for (int c = 0; c < nsl; ++c) {
      const size_t a = std::min(span, (size_t)c * step), b = std::min(span, a + step);
      if (nsl > 1) CCGP_HIP(hipEventSynchronize(h->pull_ev[c]));
      else CCGP_HIP(hipStreamSynchronize(h->stream));
      for (const Piece& p : ps) {
        if (!p.host || !p.bytes) continue;
        const size_t p0 = (size_t)(static_cast<char*>(p.dev) - lo), p1 = p0 + p.bytes;
        const size_t x0 = std::max(p0, a), x1 = std::min(p1, b);
        if (x1 > x0) std::memcpy(static_cast<char*>(p.host) + (x0 - p0), pin + x0, x1 - x0);
      }
    }
    return CCGP_OK;
  }
  for (const Piece& p : ps)
    if (p.host && p.bytes) CCGP_HIP(hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDeviceToHost, h->stream));
  CCGP_HIP(hipStreamSynchronize(h->stream));
  return CCGP_OK;
}

// the `gauss` flag of the four route decisions the fused family evaluators serve (CCGP_OPT_FAMILY_FUSED: Op::Loglik,
// small_route_sets, small_route_chain, small_route_nm); every other decision asks `fam.id == 0`, but for prediction and
// leave-one-out under their own option (gauss_or_fused_predict, gauss_or_fused_loo below)
bool gauss_or_fused(const ccgp_handle* h, int n, int d, int K) {
  return h->fam.id == 0 || (h->opt_family_fused != 0 && small_family_fused_supported(h->fam.id, n, d, K));
}

// the `gauss` flags of a prediction and of leave-one-out (CCGP_OPT_FAMILY_FUSED_PREDICT): what predict_run and loo_run pass
// to small_route(Op::Predict) / kept_factor_ws_bytes and to small_route_loo, and what ccgp_reserve asks.  `fam` is the
// call's family (a factor set keeps its own).  A family has the kept-factor scheme only, so without
// CCGP_OPT_PREDICT_FACTOR its prediction stays on the sweep.
bool gauss_or_fused_predict(const ccgp_handle* h, const KernelFamily& fam, int n, int d, int K) {
  return fam.id == 0 || (h->opt_family_fused_predict != 0 && h->opt_predict_factor != 0 &&
                         small_family_fused_predict_supported(fam.id, n, d, K));
}
bool gauss_or_fused_loo(const ccgp_handle* h, const KernelFamily& fam, int n, int d, int K) {
  return fam.id == 0 || (h->opt_family_fused_predict != 0 && small_family_fused_loo_supported(fam.id, n, d, K));
}
// the `gauss` flag of ccgp_loglik_grad_batch, ccgp_profile_batch and ccgp_profile_batch_sets (CCGP_OPT_FAMILY_FUSED_GRAD): what
// grad_call and grad_run pass to small_route(Op::Grad) with a gradient and to small_route(Op::Loglik) for the value-only
// profiled call, and what ccgp_profile_batch_sets passes to small_route_profile_grad_sets.  With a gradient, false is a refusal.
bool gauss_or_fused_grad(const ccgp_handle* h, const KernelFamily& fam, int n, int d, int K, bool grad) {
  if (fam.id == 0) return true;
  if (h->opt_family_fused_grad == 0) return false;
  return grad ? small_family_fused_grad_supported(fam.id, n, d, K) : small_family_fused_profile_supported(fam.id, n, d, K);
}

bool bad_shape(int n, int d, int K) {
  return n < 1 || d < 1 || d > kMaxD || K < 1 || K > kMaxK;
}

// How many items (matrices of a blocked sweep, draws of a kept-factor prediction) one pass takes, and the workspace for
// them: as many as `per_item` bytes each allow under the workspace limit and under what the device can give right now
// (free memory plus what this handle would release by regrowing, less `margin`: other handles / processes may share
// the device), at most 65535 (the chunk index is a grid y / z dimension in cov_kernel, rhs_rows_kernel, ...), at
// least 1.  The workspace grows to total_bytes(chunk); when another handle / process took the memory in between, the
// chunk is halved until it fits.
constexpr size_t kSweepMargin = size_t(1) << 30;
constexpr size_t kFactorsetMargin = size_t(256) << 20;   // the factor set itself holds most of the device

template <class TotalBytes>
int plan_chunk(ccgp_handle* h, size_t per_item, int count, size_t margin, TotalBytes total_bytes, int* chunk) {
  size_t limit = h->ws_limit, free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    const size_t avail = free_b + h->ws.bytes > margin ? free_b + h->ws.bytes - margin : 0;
    if (avail < limit) limit = avail;
  }
  int nb = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)count, 65535), limit / per_item));
  int rc = ensure(h, h->ws, kWorkspace, total_bytes(nb));
  while (rc == CCGP_ENOMEM && nb > 1) {
    nb = (nb + 1) / 2;
    rc = ensure(h, h->ws, kWorkspace, total_bytes(nb));
  }
  *chunk = nb;
  return rc;
}

// The blocked sweep's workspace: a chunk of nb matrices of npad rows with ne extra tile rows, and behind them what
// `scratch(Layout&, nb)` declares -- once per candidate chunk size to measure, and once over the workspace, where it hands
// out its pointers.  scratch_per_item: what a matrix's share of the scratch adds to the plan's bytes per item.
template <class Scratch>
int sweep_plan(ccgp_handle* h, int npad, int ne, int count, size_t scratch_per_item, Scratch&& scratch, int* chunk) {
  auto lay = [&](Layout& w, int nb) {
    w.off += blocked_ws_bytes(npad, nb, ne);
    scratch(w, nb);
  };
  if (int rc = plan_chunk(h, blocked_ws_bytes(npad, 1, ne) + scratch_per_item, count, kSweepMargin,
                          [&](int nb) { return layout_bytes([&](Layout& w) { lay(w, nb); }); }, chunk))
    return rc;
  Layout ws(h->ws.ptr);
  lay(ws, *chunk);
  return CCGP_OK;
}

// One blocked sweep over the `count` draws of dv on resident inputs: plan the chunk, zero the status words, factorise
// chunk by chunk with `job` riding along, check the launches.  `out` and `job` are read AFTER the plan, so `scratch` may
// point them into the workspace.
template <class Scratch>
int run_sweep(ccgp_handle* h, const double* dX, int n, int d, const double* dy, const DrawView& dv, int count, int ne,
              double sigma2, int mean_mode, double tau2, const SweepOut& out, const BlockedJob* job,
              size_t scratch_per_item, Scratch&& scratch) {
  const int npad = round_up(n, kTile);
  int nbc = 0;
  if (int rc = sweep_plan(h, npad, ne, count, scratch_per_item, scratch, &nbc)) return rc;
  CCGP_HIP(hipMemsetAsync(out.status, 0, sizeof(int) * (size_t)count, h->stream));
  for (int b0 = 0; b0 < count; b0 += nbc) {
    const int nb = std::min(nbc, count - b0);
    blocked_loglik(h, dX, n, d, dy, dv, b0, nb, npad, sigma2, mean_mode, tau2, blocked_carve(h->ws.ptr, npad, nb, ne),
                   out.loglik, out.beta, out.status, job);
  }
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}
const auto no_scratch = [](Layout&, int) {};

int check_mean_mode(ccgp_handle* h, int mean_mode) {
  if (mean_mode != CCGP_MEAN_PROFILE_BETA && mean_mode != CCGP_MEAN_ZERO_PLUS_TAU2)
    return fail(h, CCGP_EINVAL, "ccgp_loglik_batch: unknown mean_mode");
  return CCGP_OK;
}

// the B >= 1 evaluations of dv on resident inputs; arguments are checked by the callers
int loglik_run(ccgp_handle* h, const double* dX, int n, int d, const double* dy, const DrawView& dv, double sigma2,
               int mean_mode, double tau2, double* d_loglik, double* d_beta, int* d_status) {
  const int K = dv.K, B = dv.ldp;
  if (small_route(Op::Loglik, gauss_or_fused(h, n, d, K), n, d, K) == Route::Blocked)
    return run_sweep(h, dX, n, d, dy, dv, B, 0, sigma2, mean_mode, tau2, {d_loglik, d_beta, d_status}, nullptr, 0, no_scratch);
  ScopedTimer t(h, CCGP_T_FUSED);
  launch_small_reg_loglik(h->stream, dX, n, d, dy, dv, B, sigma2, mean_mode, tau2, d_loglik, d_beta,
                          d_status, h->opt_small_grid16 != 0);
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}

int loglik_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
               const double* dparams, int B, double sigma2, int mean_mode, double tau2,
               double* d_loglik, double* d_beta, int* d_status) {
  if (bad_shape(n, d, K) || B < 0 || !dX || !dy || !dparams || !d_loglik || !d_status)
    return fail(h, CCGP_EINVAL, "ccgp_loglik_batch: bad argument");
  if (int rc = check_mean_mode(h, mean_mode)) return rc;
  if (B == 0) return CCGP_OK;
  DrawView dv;
  if (int rc = draw_view(h, h->fam, dparams, B, K, d, &dv)) return rc;
  return loglik_run(h, dX, n, d, dy, dv, sigma2, mean_mode, tau2, d_loglik, d_beta, d_status);
}

// The value and gradient of the B >= 1 draws of dv on resident inputs, the counterpart of loglik_run.  o.s2hat set: the
// profiled mode -- sigma2 is not read, the evaluation runs at 1.0 and leaves each draw's sigma2_hat there.  o.grad ==
// nullptr (profiled mode only): value alone, which is a likelihood call and takes the likelihood's route.  `who` names
// the entry point in a refusal; the callers have refused a gradient outside the Gaussian family and outside what
// CCGP_OPT_FAMILY_FUSED_GRAD serves.
int grad_run(ccgp_handle* h, const char* who, const double* dX, int n, int d, const double* dy, const DrawView& dv,
             double sigma2, const GradOut& o) {
  const int K = dv.K, B = dv.ldp, P = K + K * d;
  if (o.s2hat) sigma2 = 1.0;
  const Route route = small_route(o.grad ? Op::Grad : Op::Loglik, gauss_or_fused_grad(h, dv.fam, n, d, K, o.grad != nullptr), n, d, K);
  if (o.grad && route == Route::Blocked && !blocked_grad_supported(d, K))
    return fail(h, CCGP_EUNSUPPORTED, std::string(who) + ": d + K too large for the contraction kernel's LDS");
  if (route == Route::Blocked) {
    // With a gradient, identity rows ride along as extra tile rows, then the tiles of R^-1 are formed (rinv_tile_kernel),
    // turned into M and contracted with the kernel derivatives (grad_contract_kernel; blocked.hip).  Behind the chunk's
    // matrices, from the next 256-byte line: the contraction's partial sums and alpha for every matrix of the chunk.
    // Profiled: finish_kernel leaves sigma2_hat per matrix in o.s2hat (indexed by draw across the chunks, as loglik, beta
    // and status are) and the gradient stages read it there.
    const int npad = round_up(n, kTile);
    const size_t ntiles = blocked_grad_partials(npad);
    BlockedJob job{};
    job.kind = o.grad ? kJobGrad : kJobNone; job.grad = o.grad; job.Btot = B; job.s2hat = o.s2hat;
    return run_sweep(h, dX, n, d, dy, dv, B, o.grad ? npad / kTile : 0, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0,
                     {o.loglik, o.beta, o.status}, &job, o.grad ? sizeof(double) * (ntiles * P + npad) : 0,
                     [&](Layout& w, int nb) {
                       if (!o.grad) return;
                       w.off = Layout::al(w.off);
                       job.gpart = w.take<double>((size_t)nb * ntiles * P);
                       job.alpha = w.take<double>((size_t)nb * npad);
                     });
  }
  ScopedTimer t(h, CCGP_T_FUSED);
  if (route == Route::Lds)
    launch_small_grad(h->stream, dX, n, d, dy, dv, B, sigma2, o.loglik, o.beta, o.grad, o.status, o.gpart, o.s2hat);
  else if (o.s2hat)
    launch_small_reg_profile(h->stream, dX, n, d, dy, dv, B, o.loglik, o.s2hat, o.beta, o.grad, o.status, h->opt_small_grid16 != 0);
  else
    launch_small_reg_grad(h->stream, dX, n, d, dy, dv, B, sigma2, o.loglik, o.beta, o.grad, o.status);
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}

// the end of a batch call: the status words go to the caller if asked for, and the number of failed evaluations is the
// C ABI's positive return value
int report_status(const std::vector<int>& st, int* status) {
  if (status) std::memcpy(status, st.data(), sizeof(int) * st.size());
  int c = 0;
  for (int v : st) c += v != 0;
  return c;
}

// pull the result pieces and the B status words at dst, then report_status.  whole_doubles: one word more when B is odd,
// for a caller whose status words close a piece of doubles (ccgp_loglik_batch: the copy back stays a multiple of 8 bytes;
// 140 instead of 144 bytes for 7 candidates measured 1.2 us more per call)
int pull_status(ccgp_handle* h, Pieces ps, int* dst, int B, int* status, size_t pin_max = kPinMax,
                bool whole_doubles = false) {
  std::vector<int> st((size_t)B + (whole_doubles ? B & 1 : 0));
  std::vector<Piece> all;
  all.reserve((size_t)(ps.end() - ps.begin()) + 1);
  all.assign(ps.begin(), ps.end());
  all.push_back(piece(dst, st.data(), st.size()));
  if (int rc = pull(h, all, pin_max)) return rc;
  st.resize(B);
  return report_status(st, status);
}

// ccgp_loglik_grad_batch and, with out_sigma2, ccgp_profile_batch behind their argument checks: stage, push, grad_run, pull
int grad_call(ccgp_handle* h, const char* who, const double* X, int n, int d, const double* y, int K, const double* params,
              int B, double sigma2, double* out_loglik, double* out_sigma2, double* out_beta, double* out_grad, int* status) {
  // (a 1-D family under CCGP_OPT_FAMILY_FUSED_GRAD: the flag grad_run passes)
  const bool gauss = gauss_or_fused_grad(h, h->fam, n, d, K, out_grad != nullptr);
  if (out_grad && !gauss)
    return fail(h, CCGP_EUNSUPPORTED, std::string(who) + ": analytic gradient is implemented for the Gaussian family only");
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  // the partial sums of launch_small_grad: staged where grad_run takes the in-LDS route
  const bool lds = small_route(out_grad ? Op::Grad : Op::Loglik, gauss, n, d, K) == Route::Lds;
  GradStage s;
  if (int rc = stage(h, [&](Layout& c) {
        s = grad_stage(c, n, d, P, B, out_grad, out_sigma2, lds ? (size_t)B * small_grad_chunks(n, d) * P : 0);
      }))
    return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, B, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(X, y, params))) return prc;
  if (int rc = grad_run(h, who, s.X, n, d, s.y, dv, sigma2, s.o)) return rc;
  return pull_status(h, s.results(out_grad, out_loglik, out_sigma2, out_beta), s.o.status, B, status);
}

int check_summary_args(ccgp_handle* h, int m, const double* probs, int n_probs) {
  if (m < 1 || n_probs < 0 || n_probs > CCGP_SUMMARY_MAX_PROBS || (n_probs > 0 && !probs))
    return fail(h, CCGP_EINVAL, "ccgp_predict_summary: m >= 1 and 0 <= n_probs <= 8 (with probs) are required");
  for (int j = 0; j < n_probs; ++j)
    if (!(probs[j] > 0.0 && probs[j] < 1.0))
      return fail(h, CCGP_EINVAL, "ccgp_predict_summary: every level of probs must lie strictly inside (0, 1)");
  return CCGP_OK;
}

// ---- kept-factor prediction: what predict_run needs beyond the launches, shared with ccgp_reserve ---------------------
// the scratch for S draws at m test sites -- the factor block and the correlation vectors of as many draws at a time as
// half the workspace limit allows (at least 64) --, or 0 where that scheme does not serve the shape (route, option, LDS)
size_t kept_factor_ws_bytes(const ccgp_handle* h, bool gauss, int n, int d, int K, int S, int m) {
  if (!h->opt_predict_factor || small_route(Op::Predict, gauss, n, d, K) != Route::Reg || !small_reg_sites_supported(n, d, K))
    return 0;
  const size_t per = small_reg_sites_scratch(n, d, K, m);
  const size_t want = per * (size_t)S, cap = std::max<size_t>(h->ws_limit / 2, per * 64);
  return std::min(want, cap / per * per);
}
// its second stream and the fork / join events, created once per handle; false: the scheme runs on one stream
bool ensure_aux(ccgp_handle* h) {
  if (h->aux_stream) return true;
  if (hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking) != hipSuccess) h->aux_stream = nullptr;
  if (h->aux_stream && (hipEventCreateWithFlags(&h->aux_fork, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&h->aux_join, hipEventDisableTiming) != hipSuccess)) {
    (void)hipStreamDestroy(h->aux_stream);
    h->aux_stream = nullptr;
  }
  return h->aux_stream != nullptr;
}

// ---- tiny kernels for the literal R.Inv-based helpers (a6, a7, a10, a11) -----------------
// (Rounds 1 - 3 let one thread walk a whole row or column of R.Inv alone: ~20 us per kernel for 4096 multiply-adds at
// n = 64, a third of a literal call.  Now lane = row -- a column of R.Inv is contiguous --, the four waves share the columns
// and combine in LDS in fixed order.)
__device__ inline double wg4_sum(double x, double (&red)[4], int tid) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void rinv_terms_kernel(const double* Rinv, const double* y, int n, double beta,
                                                         double* mean_factor, double* colsum, double* scal) {
  // one workgroup; scal[0] = 1'Rinv y, scal[1] = sum(Rinv), scal[2] = (y-b)'Rinv(y-b).
  // The caller's R.Inv is taken as it is, symmetric or not (R's solve() output is symmetric only up to rounding):
  // var.factor1 = apply(R.Inv, 2, sum) are COLUMN sums (HX:609), 1'R.Inv y = sum_j colsum_j y_j (HX:387), and
  // mean.factor = R.Inv %*% (y - beta) are row dot products (HX:608).
  __shared__ double part[4][64];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    // rows i0 .. i0 + 63: (R.Inv (y - beta))_i, lane = row (a column of R.Inv is contiguous), the waves share the columns
    const int i = i0 + lane;
    double mf = 0.0;
    if (i < n) {
#pragma unroll 4
      for (int j = wave; j < n; j += 4) mf = fma(Rinv[i + (size_t)j * n], y[j] - beta, mf);
    }
    part[wave][lane] = mf;
    __syncthreads();
    if (wave == 0 && i < n) {
      mf = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      if (mean_factor) mean_factor[i] = mf;
      a2 += (y[i] - beta) * mf;
    }
    __syncthreads();
  }
  // column sums: four lanes per column (rows i = q, q + 4, ...), combined in fixed order
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + (tid >> 2), q = tid & 3;
    double cs = 0.0;
    if (j < n) {
      const double* col = Rinv + (size_t)j * n;
#pragma unroll 4
      for (int i = q; i < n; i += 4) cs += col[i];
    }
    cs += __shfl_xor(cs, 1, 64);
    cs += __shfl_xor(cs, 2, 64);
    if (j < n && q == 0) {
      if (colsum) colsum[j] = cs;
      a0 += cs * y[j];
      a1 += cs;
    }
  }
  a0 = wg4_sum(a0, red, tid);
  a1 = wg4_sum(a1, red, tid);
  a2 = wg4_sum(a2, red, tid);
  if (tid == 0) { scal[0] = a0; scal[1] = a1; scal[2] = a2; }
}

__global__ __launch_bounds__(256) void predict_factors_kernel(const double* r, int m, int n, double beta,
                                                              const double* mean_factor, const double* v1, double v2,
                                                              const double* Rinv, double sigma2, double* mean, double* var) {
  // one workgroup per test point t; r is m x n column-major (r[t + i*m])
  __shared__ double part[4][64];
  __shared__ double red[4];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double q = 0.0, s1 = 0.0, sm = 0.0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    double acc = 0.0;
    if (i < n) {
#pragma unroll 4
      for (int j = wave; j < n; j += 4) acc = fma(Rinv[i + (size_t)j * n], r[t + (size_t)j * m], acc);
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && i < n) {
      acc = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      const double ri = r[t + (size_t)i * m];
      q = fma(ri, acc, q);
      s1 = fma(v1[i], ri, s1);
      sm = fma(mean_factor[i], ri, sm);
    }
    __syncthreads();
  }
  q = wg4_sum(q, red, tid);
  s1 = wg4_sum(s1, red, tid);
  sm = wg4_sum(sm, red, tid);
  if (tid == 0) {
    const double u = 1.0 - s1;
    var[t] = sigma2 * (1.0 - q + u * u / v2);
    mean[t] = beta + sm;
  }
}

// log-mean-exp of each grid row's N conditional log-likelihoods (likeli.hyperpars, HX:574):
// logs is laid out [g*N + j]; NaN entries (non-PD draws) propagate as in R's mean().
__global__ void row_logmeanexp_kernel(const double* logs, int N, int take_log, double* out) {
  __shared__ double red[4];
  const int g = blockIdx.x, tid = threadIdx.x;
  const double* row = logs + (size_t)g * N;
  double mx = -INFINITY;
  bool nan = false;
  for (int j = tid; j < N; j += blockDim.x) {
    double v = row[j];
    if (v != v) nan = true;
    mx = fmax(mx, v);
  }
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_down(mx, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  double s = 0.0;
  for (int j = tid; j < N; j += blockDim.x) s += exp(row[j] - mx);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  int anynan = __syncthreads_or(nan ? 1 : 0);
  if (tid == 0) {
    double tot = red[0] + red[1] + red[2] + red[3];
    double lme = mx + log(tot / N);
    double v = take_log ? lme : exp(lme);
    if (anynan) v = __longlong_as_double(0x7ff8000000000000LL);
    out[g] = v;
  }
}

// ---- hyperprior grid: the G x N table of draws, built on the device (likeli.hyperpars HX:554-559) ----------
// qtab[s * N + j] = qgamma(1 - u_j, shape_s, rate 1),  u_j = runif.halton(N, 1)[j]
__global__ void grid_qtab_kernel(const double* shapes, int ns, int N, double* qtab) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ns * N) return;
  const int s = (int)(idx / N), j = (int)(idx % N);
  qtab[idx] = qgamma_unit(1.0 - halton2((unsigned)j + 1u), shapes[s]);
}

// draw b = g N + j: p = u_j, theta1 = qigamma(u_j, a1, b1) = b1 / qtab[a1][j], theta2 likewise (HX:554-556);
// isotropic: theta_c repeated over the d dimensions; anisotropic (ANI:399-406 with the grid's quantiles per
// dimension, BASELINE config 3): component 1 = (theta1, theta2), component 2 = (1 + lambda) (theta1, theta2)
__global__ void grid_expand_kernel(const double* hyper, const int* shape_idx, const double* qtab, int G, int N,
                                   int d, int aniso, double lambda, double* params) {
  const size_t B = (size_t)G * N;
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int g = (int)(b / N), j = (int)(b % N);
  const double p = halton2((unsigned)j + 1u);
  const double th1 = hyper[g + (size_t)G] / qtab[(size_t)shape_idx[g] * N + j];
  const double th2 = hyper[g + (size_t)3 * G] / qtab[(size_t)shape_idx[G + g] * N + j];
  params[b] = p;
  params[b + B] = 1.0 - p;
  if (aniso) {
    params[b + 2 * B] = th1;
    params[b + 3 * B] = th2;
    params[b + 4 * B] = (1.0 + lambda) * th1;
    params[b + 5 * B] = (1.0 + lambda) * th2;
  } else {
    for (int k = 0; k < d; ++k) {
      params[b + (size_t)(2 + k) * B] = th1;
      params[b + (size_t)(2 + d + k) * B] = th2;
    }
  }
}

// number of evaluations whose factorisation met a non-positive pivot (the C ABI's positive return value)
__global__ void count_bad_kernel(const int* status, int B, int* out) {
  int c = 0;
  const int end = min(B, (int)(blockIdx.x + 1) * 1024);
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < end; i += 256) c += status[i] != 0;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// The fallback where the sets kernel has no route: the rows of every set, in their order, through a single-set call.
// call(c, rows, nb, idx) evaluates the nb rows of set c (column-major, leading dimension nb) and scatters its results by
// idx, the rows' places among the B; it returns what the single-set entry point returned.
template <class Call>
int sets_by_group(const int* set, int B, int C, int P, const double* params, Call call) {
  std::vector<std::vector<int>> rows_of(C);
  for (int b = 0; b < B; ++b) rows_of[set[b]].push_back(b);
  int failed = 0;
  std::vector<double> rows;
  for (int c = 0; c < C; ++c) {
    const std::vector<int>& idx = rows_of[c];
    const int nb = (int)idx.size();
    if (!nb) continue;
    rows.resize((size_t)nb * P);
    for (int j = 0; j < P; ++j)
      for (int i = 0; i < nb; ++i) rows[i + (size_t)j * nb] = params[idx[i] + (size_t)j * B];
    const int rc = call(c, rows.data(), nb, idx);
    if (rc < 0) return rc;
    failed += rc;
  }
  return failed;
}
// out[idx[i] + j * ldo] = src[i + j * nb] for the P columns of a group's result; out == nullptr: not wanted
template <class T>
void scatter_by(const std::vector<int>& idx, const std::vector<T>& src, T* out, int P = 1, int ldo = 0) {
  const size_t nb = idx.size();
  if (!out) return;
  for (int j = 0; j < P; ++j)
    for (size_t i = 0; i < nb; ++i) out[idx[i] + (size_t)j * ldo] = src[i + (size_t)j * nb];
}

// row b0 of a per-row array; nullptr stays nullptr (an input the call does not take, an output the caller does not want)
template <class T>
T* at(T* p, int b0) {
  return p ? p + b0 : nullptr;
}

// rows b0 .. b0 + nb of a B x P column-major table as an nb x P one: `rows` where the chunk is not the whole table
const double* chunk_rows(const double* params, int B, int P, int b0, int nb, std::vector<double>& rows) {
  if (nb == B) return params;
  rows.resize((size_t)nb * P);
  for (int j = 0; j < P; ++j) std::memcpy(&rows[(size_t)j * nb], params + b0 + (size_t)j * B, sizeof(double) * nb);
  return rows.data();
}

// A call of B rows cut into chunks.  A chunk is a call of its own: stage(Layout&, nb) lays out, in the workspace, what the
// whole call shares and behind it a chunk's rows and results (row_bytes each).  The planner cuts B by the workspace limit
// and by the grid's 65535; a row reads its own parameters (and its own set) only, so where the cuts fall changes no bit.
// body(s, b0, nb, rows, table) pushes, launches and returns pull_status's value for rows b0 .. b0 + nb: rows is their
// nb x P column-major parameter table, table where their nb x P result table goes when the caller wants one (out_table,
// B x P column-major) -- out_table itself for an uncut call, else a buffer this runner scatters into out_table's rows.
template <class Stage, class Body>
int run_chunked(ccgp_handle* h, size_t row_bytes, const double* params, int B, int P, double* out_table, Stage stage,
                Body body) {
  int nbc = 0;
  if (int rc = plan_chunk(h, row_bytes, B, kSweepMargin,
                          [&](int nb) { return layout_bytes([&](Layout& w) { stage(w, nb); }); }, &nbc))
    return rc;
  Layout ws(h->ws.ptr);
  const auto s = stage(ws, nbc);
  std::vector<double> rows, table;
  int failed = 0;
  for (int b0 = 0; b0 < B; b0 += nbc) {
    const int nb = std::min(nbc, B - b0);
    const bool cut = out_table && nb != B;
    if (cut) table.resize((size_t)nb * P);
    const int rc = body(s, b0, nb, chunk_rows(params, B, P, b0, nb, rows), cut ? table.data() : out_table);
    if (rc < 0) return rc;
    failed += rc;
    if (cut)
      for (int j = 0; j < P; ++j) std::memcpy(out_table + b0 + (size_t)j * B, &table[(size_t)j * nb], sizeof(double) * nb);
  }
  return failed;
}

// One transformed parameter vector (psi1, psi2, phi[, zeta]) = (log theta1, log theta2, logit p[, log lambda]) -> the C-ABI
// parameter row (w_1, w_2, theta_1k.., theta_2k..), the log-Jacobian and the script's log-prior (HX:446-463, GV:450, ISO:453,
// ANI:459-462).  theta_t / row: element j of vector b at [b + j * ld]; shared by ccgp_logpost and ccgp_logpost_batch so that a
// value does not depend on which of the two produced it.
void logpost_terms(int prior_id, int d, const double* theta_t, int ldt, const double* prior_pars, double* row, int ldr,
                   double* log_jacob, double* log_prior) {
  const double psi1 = theta_t[0], psi2 = theta_t[ldt], phi = theta_t[2 * (size_t)ldt];
  const double theta1 = std::exp(psi1), theta2 = std::exp(psi2);
  const double p = 1.0 / (1.0 + std::exp(-phi));
  row[0] = p;
  row[ldr] = 1.0 - p;
  double lj = -phi - 2.0 * std::log(1.0 + std::exp(-phi)) + psi1 + psi2;
  double lp = 0.0;
  if (prior_id == CCGP_PRIOR_ANI) {
    const double zeta = theta_t[3 * (size_t)ldt], lambda = std::exp(zeta);
    row[2 * (size_t)ldr] = theta1; row[3 * (size_t)ldr] = theta2;
    row[4 * (size_t)ldr] = (1.0 + lambda) * theta1; row[5 * (size_t)ldr] = (1.0 + lambda) * theta2;
    lj += zeta;
    lp = -psi1 - psi1 * psi1 / 2.0 - psi2 - psi2 * psi2 / 2.0 - 4.0 * zeta - 4.0 / lambda;
  } else {
    for (int k = 0; k < d; ++k) { row[(size_t)(2 + k) * ldr] = theta1; row[(size_t)(2 + d + k) * ldr] = theta2; }
    if (prior_id == CCGP_PRIOR_INVGAMMA)
      lp = -(prior_pars[0] + 1.0) * psi1 - prior_pars[1] / theta1 -
           (prior_pars[2] + 1.0) * psi2 - prior_pars[3] / theta2;
    else if (prior_id == CCGP_PRIOR_GV)
      lp = -4.0 * psi1 - 1.0 / theta1 - 6.0 * psi2 - 75.0 / theta2;
    else
      lp = -4.0 * psi1 - 2.0 / theta1 - 6.0 * psi2 - 16.0 / theta2;
  }
  *log_jacob = lj;
  *log_prior = lp;
}

// ccgp_logpost_batch and ccgp_logpost_sets behind their argument checks: logpost_terms over the B vectors of theta_t,
// loglik(K, rows, ll, beta, st) -> the likelihood call's return value, then the sums in ccgp_logpost's order of additions
// (NaN where the factorisation failed: the reference's NA)
template <class Loglik>
int logpost_rows(int prior_id, int d, const double* theta_t, int B, const double* prior_pars, double* out_val,
                 double* out_beta, double* out_loglik, int* status, Loglik loglik) {
  const int K = 2, P = K + K * d;
  std::vector<double> rows((size_t)B * P), ljac(B), lpri(B), ll(B), beta(B);
  std::vector<int> st(B);
  for (int b = 0; b < B; ++b) logpost_terms(prior_id, d, theta_t + b, B, prior_pars, rows.data() + b, B, &ljac[b], &lpri[b]);
  const int rc = loglik(K, rows.data(), ll.data(), beta.data(), st.data());
  if (rc < 0) return rc;
  for (int b = 0; b < B; ++b) {
    out_val[b] = ll[b] + ljac[b] + lpri[b];
    if (out_beta) out_beta[b] = beta[b];
    if (out_loglik) out_loglik[b] = ll[b];
    if (status) status[b] = st[b];
  }
  return rc;
}

// ---- the portable terms (chain_terms.h) on the host: the twin of what the chain kernel computes ---------------------------
struct ChainTables {
  double hi[kChainTable], lo[kChainTable];
  ChainTables() {
    static const unsigned long long hb[kChainTable] = CCGP_EXP_TABLE_BITS, lb[kChainTable] = CCGP_CHAIN_EXP_LO_BITS;
    for (int j = 0; j < kChainTable; ++j) { hi[j] = chain_from_bits(hb[j]); lo[j] = chain_from_bits(lb[j]); }
  }
};
const ChainTables& chain_tables() {
  static const ChainTables t;
  return t;
}
// logpost_terms' outputs for the B vectors of theta_t (B x q column-major) by chain_terms: rows B x P column-major
void chain_terms_rows(int prior_id, int d, const double* theta_t, int B, const double* prior_pars, double* rows, double* ljac,
                      double* lpri) {
  const ChainTables& tb = chain_tables();
  const int q = prior_id == CCGP_PRIOR_ANI ? 4 : 3;
  for (int b = 0; b < B; ++b) {
    double th[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < q; ++j) th[j] = theta_t[b + (size_t)j * B];
    const ChainTerms tm = chain_terms(prior_id, th, prior_pars, tb.hi, tb.lo);
    rows[b] = tm.w0;
    rows[b + (size_t)B] = tm.w1;
    for (int c = 0; c < 2; ++c)
      for (int k = 0; k < d; ++k) rows[b + (size_t)(2 + c * d + k) * B] = chain_rate(tm, prior_id, c, k);
    ljac[b] = tm.lj;
    lpri[b] = tm.lp;
  }
}
// what ccgp_logpost_batch refuses about a prior, without a handle to carry the message
bool chain_prior_ok(int prior_id, int d, const double* prior_pars) {
  if (prior_id < CCGP_PRIOR_INVGAMMA || prior_id > CCGP_PRIOR_ANI) return false;
  if (prior_id == CCGP_PRIOR_INVGAMMA && !prior_pars) return false;
  return prior_id != CCGP_PRIOR_ANI || d == 2;
}

}  // namespace

// No C++ exception may cross the C ABI (inside R that would be std::terminate for the user's session): every entry point
// that takes a handle is a function-try-block; host-memory exhaustion (std::vector / std::string growth) comes back as
// CCGP_ENOMEM, anything else as CCGP_EHIP, with the message in ccgp_last_error.
#define CCGP_GUARD_END(h)                                                                    \
  catch (const std::bad_alloc&) {                                                            \
    return fail_noexcept(h, CCGP_ENOMEM, "host memory exhausted inside libccgp");            \
  } catch (const std::exception& e_) {                                                       \
    return fail_noexcept(h, CCGP_EHIP, e_.what());                                           \
  } catch (...) {                                                                            \
    return fail_noexcept(h, CCGP_EHIP, "unknown C++ exception inside libccgp");              \
  }

extern "C" {

const char* ccgp_version(void) { return "ccgp-mi355x 0.1 (gfx950)"; }

int ccgp_create(int device, ccgp_handle** out) {
  if (!out) return CCGP_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return CCGP_EHIP;
  if (hipSetDevice(device) != hipSuccess) return CCGP_EHIP;
  ccgp_handle* h = new (std::nothrow) ccgp_handle();
  if (!h) return CCGP_ENOMEM;
  h->device = device;
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return CCGP_EHIP;
  }
  h->stream = h->own_stream;
  // default scratch cap: three quarters of the device (216 of 288 GB on MI355X -- the whole 512-point
  // n = 4096 grid of BASELINE config 4 is 73 GB and runs as ONE chunk)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) h->ws_limit = total_b / 4 * 3;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_cus = cus;
  if (const char* e = std::getenv("CCGP_SCHED_BACKLOG")) h->sched_backlog_min = std::atoi(e);
  if (const char* e = std::getenv("CCGP_SCHED_TIMEOUT_MS")) {
    const int v = std::atoi(e);
    if (v > 0) h->sched_timeout_ms = v;
  }
  *out = h;
  return CCGP_OK;
}

int ccgp_destroy(ccgp_handle* h) try {
  if (!h) return CCGP_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  for (auto& s : h->spans) {
    (void)hipEventDestroy(s.e0);
    (void)hipEventDestroy(s.e1);
  }
  if (h->ws.ptr) (void)kWorkspace.release(h->ws.ptr);
  if (h->stage.ptr) (void)kStaging.release(h->stage.ptr);
  if (h->pin.ptr) (void)kPinned.release(h->pin.ptr);
  for (auto& e : h->pull_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->aux_fork) (void)hipEventDestroy(h->aux_fork);
  if (h->aux_join) (void)hipEventDestroy(h->aux_join);
  if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return CCGP_OK;
} CCGP_GUARD_END(h)

const char* ccgp_last_error(const ccgp_handle* h) { return h ? h->err.c_str() : "null handle"; }

int ccgp_set_stream(ccgp_handle* h, void* hip_stream) try {
  if (!h) return CCGP_EINVAL;
  h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_set_kernel(ccgp_handle* h, int family, double nu) try {
  if (!h) return CCGP_EINVAL;
  if (family == CCGP_KERNEL_GAUSS) {
    h->fam = ccgp::KernelFamily{};
    return CCGP_OK;
  }
  if ((family != CCGP_KERNEL_MATERN && family != CCGP_KERNEL_MATERN_SPLINE) || !(nu > 1.0) || !(nu <= 10.0))
    return fail(h, CCGP_EINVAL, "ccgp_set_kernel: family must be CCGP_KERNEL_GAUSS, or CCGP_KERNEL_MATERN / CCGP_KERNEL_MATERN_SPLINE with 1 < nu <= 10 (the range the quadrature is validated on; the scripts use 5)");
  h->fam.id = family;
  h->fam.nu = nu;
  h->fam.norm = 1.0 / (std::tgamma(nu) * std::pow(2.0, nu - 1.0));
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_set_workspace_limit(ccgp_handle* h, size_t bytes) try {
  if (!h || bytes < (size_t(1) << 20)) return CCGP_EINVAL;
  h->ws_limit = bytes;
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_set_option(ccgp_handle* h, int option, int value) try {
  if (!h) return CCGP_EINVAL;
  if (option == CCGP_OPT_TAIL_STRIPS && value >= 0 && value <= 2) {
    h->opt_tail_strips = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_FUSE_DIAG && (value == 0 || value == 1)) {
    h->opt_fuse_diag = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_WIDE_OFFSETS && (value == 0 || value == 1)) {
    h->opt_wide_offsets = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_SMALL_GRID16 && (value == 0 || value == 1)) {
    h->opt_small_grid16 = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_PREDICT_FACTOR && (value == 0 || value == 1)) {
    h->opt_predict_factor = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_SCHED && value >= 0 && value <= 3) {
    h->opt_sched = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_FUSED_SOLVE && value >= 0 && value <= 2) {
    h->opt_fused_solve = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_SCHED_POLICY && value >= 0 && value <= 31) {
    h->opt_sched_policy = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_FAMILY_FUSED && (value == 0 || value == 1)) {
    h->opt_family_fused = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_FAMILY_FUSED_PREDICT && (value == 0 || value == 1)) {
    h->opt_family_fused_predict = value;
    return CCGP_OK;
  }
  if (option == CCGP_OPT_FAMILY_FUSED_GRAD && (value == 0 || value == 1)) {
    h->opt_family_fused_grad = value;
    return CCGP_OK;
  }
  return fail(h, CCGP_EINVAL, "ccgp_set_option: unknown option or value");
} CCGP_GUARD_END(h)

int ccgp_synchronize(ccgp_handle* h) try {
  if (!h) return CCGP_EINVAL;
  CCGP_HIP(hipStreamSynchronize(h->stream));
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_reserve(ccgp_handle* h, int n, int d, int K, int B, int m) try {
  if (!h || bad_shape(n, d, K) || B < 1 || m < 0) return fail(h, CCGP_EINVAL, "ccgp_reserve: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  // the sweep's workspace where the likelihood or, with test sites, the prediction of this shape takes the sweep (a
  // prediction on the register-resident evaluator implies the likelihood there: its instance is the larger one)
  // (a 1-D family under CCGP_OPT_FAMILY_FUSED_PREDICT: the flag predict_run passes)
  const bool gauss = gauss_or_fused_predict(h, h->fam, n, d, K);
  const bool sweep_predict = m > 0 && small_route(Op::Predict, gauss, n, d, K) == Route::Blocked;
  if (sweep_predict || small_route(Op::Loglik, gauss_or_fused(h, n, d, K), n, d, K) == Route::Blocked) {
    int nbc = 0;
    if (int rc = sweep_plan(h, round_up(n, kTile), sweep_predict ? (m + kTile - 1) / kTile : 0, B, 0,
                            [&](Layout& t, int) { if (sweep_predict) predict_tail(t, B, nullptr, nullptr); }, &nbc))
      return rc;
  }
  // kept-factor prediction: its scratch (the size predict_run asks for) and its second stream with the two events
  if (m > 0) {
    if (const size_t want = kept_factor_ws_bytes(h, gauss, n, d, K, B, m)) {
      if (int rc = ensure(h, h->ws, kWorkspace, want)) return rc;
      if (!ensure_aux(h)) return fail(h, CCGP_EHIP, "ccgp_reserve: the second stream of the kept-factor prediction could not be created");
    }
  }
  // staging: the host-pointer likelihood and prediction, and the tables of ccgp_predict_summary_dev
  return ensure(h, h->stage, kStaging, reserve_stage_bytes(n, d, K + K * d, B, m));
} CCGP_GUARD_END(h)

int ccgp_enable_timing(ccgp_handle* h, int on) try {
  if (!h) return CCGP_EINVAL;
  // on = 1: every launch group; otherwise a bit mask, bit (1 + id) selects CCGP_T_<id> (bench.py times only
  // the update launches inside its timed region: two event records per launch are not free)
  h->timing = on == 1 ? ~0u : (unsigned)on >> 1;
  h->spans_used = 0;
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_get_timing(ccgp_handle* h, int id, double* out_ms, int* out_launches) try {
  if (!h || id < 0 || id >= CCGP_T_COUNT) return CCGP_EINVAL;
  CCGP_HIP(hipStreamSynchronize(h->stream));
  double ms = 0.0;
  int cnt = 0;
  for (size_t i = 0; i < h->spans_used; ++i) {
    if (h->spans[i].id != id) continue;
    float f = 0.f;
    CCGP_HIP(hipEventElapsedTime(&f, h->spans[i].e0, h->spans[i].e1));
    ms += f;
    ++cnt;
  }
  if (out_ms) *out_ms = ms;
  if (out_launches) *out_launches = cnt;
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_last_sched_profile(ccgp_handle* h, unsigned long long* out, int max_workgroups, int* out_workgroups) try {
  if (!h || !out || max_workgroups < 1) return CCGP_EINVAL;
  CCGP_HIP(hipSetDevice(h->device));
  // sched_prof_wgs > 0 only while the account exists: a sweep without policy bit 2 records 0, and whoever frees the
  // memory the account lies in forgets it (forget_sched_profile)
  const int nw = std::min(max_workgroups, h->sched_prof_wgs);
  if (out_workgroups) *out_workgroups = nw;
  return pull(h, {piece(h->sched_prof_dev, out, 8 * (size_t)std::max(nw, 0))});
} CCGP_GUARD_END(h)

int ccgp_debug_fill_scratch(ccgp_handle* h, int byte) try {
  if (!h) return CCGP_EINVAL;
  if (byte < -1 || byte > 255) return fail(h, CCGP_EINVAL, "ccgp_debug_fill_scratch: byte must be -1 (off) or 0 .. 255");
  h->debug_fill = byte;
  if (byte < 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  // the scheduler's time account lies in the workspace (or in a factor set, which is not the handle's to fill: that
  // account stays)
  forget_sched_profile(h, h->ws.ptr, h->ws.bytes);
  if (int rc = debug_fill(h, h->ws.ptr, h->ws.bytes, false, byte)) return rc;
  if (int rc = debug_fill(h, h->stage.ptr, h->stage.bytes, false, byte)) return rc;
  return debug_fill(h, h->pin.ptr, h->pin.bytes, true, byte);
} CCGP_GUARD_END(h)

int ccgp_workspace_bytes(const ccgp_handle* h, size_t* ws_bytes, size_t* stage_bytes) {
  if (!h) return CCGP_EINVAL;
  if (ws_bytes) *ws_bytes = h->ws.bytes;
  if (stage_bytes) *stage_bytes = h->stage.bytes;
  return CCGP_OK;
}

// ---- a1-a5 ------------------------------------------------------------------------------
static int corr_common(ccgp_handle* h, const double* Xnew, int m, const double* X, int n, int d,
                       int K, const double* params_row, double* out, bool gram) {
  if (!h || bad_shape(n, d, K) || m < 1 || !X || !params_row || !out || (!gram && !Xnew))
    return fail(h, CCGP_EINVAL, "ccgp_corr_*: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  double *dX, *dXn, *dp, *dout;
  if (int rc = stage(h, [&](Layout& c) {
        dX = c.take<double>((size_t)n * d);
        dXn = c.take<double>((size_t)m * d);
        dp = c.take<double>(P);
        dout = c.take<double>((size_t)m * n);
      }))
    return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
  if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dXn, gram ? nullptr : Xnew, (size_t)m * d), piece(dp, params_row, P)}))
    return prc;
  {
    ScopedTimer t(h, CCGP_T_COV);
    launch_cov_dense(h->stream, gram ? dX : dXn, m, dX, n, d, dv, 0, dout, m);
  }
  CCGP_LAUNCH_CHECK();
  return pull(h, {piece(dout, out, (size_t)m * n)});
}

int ccgp_corr_matrix(ccgp_handle* h, const double* X, int n, int d, const double* theta,
                     double* out_R) try {
  if (!theta || d < 1 || d > kMaxD) return fail(h, CCGP_EINVAL, "ccgp_corr_matrix: bad argument");
  std::vector<double> row(1 + d);
  row[0] = 1.0;
  for (int k = 0; k < d; ++k) row[1 + k] = theta[k];
  return corr_common(h, nullptr, n, X, n, d, 1, row.data(), out_R, true);
} CCGP_GUARD_END(h)

int ccgp_corr_cross(ccgp_handle* h, const double* Xnew, int m, const double* X, int n, int d,
                    const double* theta, double* out) try {
  if (!theta || d < 1 || d > kMaxD) return fail(h, CCGP_EINVAL, "ccgp_corr_cross: bad argument");
  std::vector<double> row(1 + d);
  row[0] = 1.0;
  for (int k = 0; k < d; ++k) row[1 + k] = theta[k];
  return corr_common(h, Xnew, m, X, n, d, 1, row.data(), out, false);
} CCGP_GUARD_END(h)

int ccgp_family_corr_dtheta(ccgp_handle* h, const double* X, int n, int K, const double* params, int q, double* out) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, 1, K) || !X || !params || !out || q < 0 || q >= K)
    return fail(h, CCGP_EINVAL, "ccgp_family_corr_dtheta: bad argument");
  if (h->fam.id == 0)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_family_corr_dtheta: the derivative table exists for CCGP_KERNEL_MATERN and CCGP_KERNEL_MATERN_SPLINE only");
  CCGP_HIP(hipSetDevice(h->device));
  double *dX, *dp, *dout;
  if (int rc = stage(h, [&](Layout& c) {
        dX = c.take<double>(n);
        dp = c.take<double>(2 * K);
        dout = c.take<double>((size_t)n * n);
      }))
    return rc;
  DrawView dv;   // the family's own refusals (K = 2 under the two-family kernel), before anything is copied
  if (int frc = draw_view(h, h->fam, dp, 1, K, 1, &dv)) return frc;
  if (int prc = push(h, {piece(dX, X, n), piece(dp, params, 2 * K)})) return prc;
  {
    ScopedTimer t(h, CCGP_T_COV);
    launch_family_dcorr(h->stream, dX, n, params[K + q], q, dv.fam, dout);
  }
  CCGP_LAUNCH_CHECK();
  return pull(h, {piece(dout, out, (size_t)n * n)});
} CCGP_GUARD_END(h)

int ccgp_mixed_corr_matrix(ccgp_handle* h, const double* X, int n, int d, int K,
                           const double* params, double* out_R) try {
  return corr_common(h, nullptr, n, X, n, d, K, params, out_R, true);
} CCGP_GUARD_END(h)

int ccgp_mixed_corr_cross(ccgp_handle* h, const double* Xnew, int m, const double* X, int n,
                          int d, int K, const double* params, double* out) try {
  return corr_common(h, Xnew, m, X, n, d, K, params, out, false);
} CCGP_GUARD_END(h)

// ---- a6, a7, a10 ---------------------------------------------------------------------------
static int rinv_terms(ccgp_handle* h, const double* R_inv, const double* y, int n, double beta,
                      double* mean_factor, double* colsum, double scal[3]) {
  if (!h || n < 1 || !R_inv || !y) return fail(h, CCGP_EINVAL, "R.Inv helper: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  double *dR, *dy, *dmf, *dcs, *dsc;
  if (int rc = stage(h, [&](Layout& c) {
        dR = c.take<double>((size_t)n * n);
        dy = c.take<double>(n);
        dmf = c.take<double>(n);
        dcs = c.take<double>(n);
        dsc = c.take<double>(4);
      }))
    return rc;
  if (int prc = push(h, {piece(dR, R_inv, (size_t)n * n), piece(dy, y, n)})) return prc;
  hipLaunchKernelGGL(rinv_terms_kernel, dim3(1), dim3(256), 0, h->stream, dR, dy, n, beta, dmf, dcs, dsc);
  CCGP_LAUNCH_CHECK();
  return pull(h, {piece(dmf, mean_factor, n), piece(dcs, colsum, n), piece(dsc, scal, 3)});
}

int ccgp_beta_mle(ccgp_handle* h, const double* R_inv, const double* y, int n, double* out_beta) try {
  if (!out_beta) return fail(h, CCGP_EINVAL, "ccgp_beta_mle: bad argument");
  double sc[3];
  int rc = rinv_terms(h, R_inv, y, n, 0.0, nullptr, nullptr, sc);
  if (rc) return rc;
  *out_beta = sc[0] / sc[1];
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_sigma2_mle(ccgp_handle* h, const double* R_inv, const double* y, int n, double beta,
                    double* out_sigma2) try {
  if (!out_sigma2) return fail(h, CCGP_EINVAL, "ccgp_sigma2_mle: bad argument");
  double sc[3];
  int rc = rinv_terms(h, R_inv, y, n, beta, nullptr, nullptr, sc);
  if (rc) return rc;
  *out_sigma2 = sc[2] / n;
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_factors(ccgp_handle* h, const double* R_inv, double beta, const double* y, int n,
                 double* out) try {
  if (!out) return fail(h, CCGP_EINVAL, "ccgp_factors: bad argument");
  double sc[3];
  int rc = rinv_terms(h, R_inv, y, n, beta, out, out + n, sc);
  if (rc) return rc;
  out[2 * n] = sc[1];
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_predict_from_factors(ccgp_handle* h, const double* r, int m, int n, double beta,
                              const double* mean_factor, const double* var_factor1,
                              double var_factor2, const double* R_inv, double sigma2,
                              double* out_mean, double* out_var) try {
  if (!h || m < 1 || n < 1 || !r || !mean_factor || !var_factor1 || !R_inv || !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_predict_from_factors: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  double *dR, *dr, *dmf, *dv1, *dmean, *dvar;
  if (int rc = stage(h, [&](Layout& c) {
        dR = c.take<double>((size_t)n * n);
        dr = c.take<double>((size_t)m * n);
        dmf = c.take<double>(n);
        dv1 = c.take<double>(n);
        dmean = c.take<double>(m);
        dvar = c.take<double>(m);
      }))
    return rc;
  if (int prc = push(h, {piece(dR, R_inv, (size_t)n * n), piece(dr, r, (size_t)m * n), piece(dmf, mean_factor, n),
                         piece(dv1, var_factor1, n)}))
    return prc;
  hipLaunchKernelGGL(predict_factors_kernel, dim3(m), dim3(256), 0, h->stream, dr, m, n, beta, dmf,
                     dv1, var_factor2, dR, sigma2, dmean, dvar);
  CCGP_LAUNCH_CHECK();
  return pull(h, {piece(dmean, out_mean, m), piece(dvar, out_var, m)});
} CCGP_GUARD_END(h)

int ccgp_predict_post(ccgp_handle* h, const double* Xnew, int m, const double* X, int n, int d, int K,
                      const double* params_row, double beta, const double* mean_factor,
                      const double* var_factor1, double var_factor2, const double* R_inv, double sigma2,
                      double* out_mean, double* out_var) try {
  if (!h || bad_shape(n, d, K) || m < 1 || !Xnew || !X || !params_row || !mean_factor || !var_factor1 || !R_inv ||
      !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_predict_post: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  double *dX, *dXn, *dp, *dmf, *dv1, *dR, *dr, *dmean, *dvar;
  if (int rc = stage(h, [&](Layout& c) {
        dX = c.take<double>((size_t)n * d);
        dXn = c.take<double>((size_t)m * d);
        dp = c.take<double>(P);
        dmf = c.take<double>(n);
        dv1 = c.take<double>(n);
        dR = c.take<double>((size_t)n * n);
        dr = c.take<double>((size_t)m * n);
        dmean = c.take<double>(m);
        dvar = c.take<double>(m);
      }))
    return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
  if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dXn, Xnew, (size_t)m * d), piece(dp, params_row, P),
                         piece(dmf, mean_factor, n), piece(dv1, var_factor1, n), piece(dR, R_inv, (size_t)n * n)}))
    return prc;
  {
    ScopedTimer t(h, CCGP_T_COV);   // r = Mixed.corr.vec(x_t, D.train, ...) (HX:665), exactly ccgp_mixed_corr_cross's kernel
    launch_cov_dense(h->stream, dXn, m, dX, n, d, dv, 0, dr, m);
  }
  hipLaunchKernelGGL(predict_factors_kernel, dim3(m), dim3(256), 0, h->stream, dr, m, n, beta, dmf, dv1,
                     var_factor2, dR, sigma2, dmean, dvar);
  CCGP_LAUNCH_CHECK();
  return pull(h, {piece(dmean, out_mean, m), piece(dvar, out_var, m)});
} CCGP_GUARD_END(h)

// ---- a8/a9/a12 -------------------------------------------------------------------------------
int ccgp_loglik_batch_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                          const double* dparams, int B, double sigma2, int mean_mode, double tau2,
                          double* d_loglik, double* d_beta, int* d_status) try {
  if (!h) return CCGP_EINVAL;
  CCGP_HIP(hipSetDevice(h->device));
  return loglik_dev(h, dX, n, d, dy, K, dparams, B, sigma2, mean_mode, tau2, d_loglik, d_beta,
                    d_status);
} CCGP_GUARD_END(h)

int ccgp_loglik_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                      const double* params, int B, double sigma2, int mean_mode, double tau2,
                      double* out_loglik, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 0 || !X || !y || !params || !out_loglik)
    return fail(h, CCGP_EINVAL, "ccgp_loglik_batch: bad argument");
  if (B == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  if (int rc = check_mean_mode(h, mean_mode)) return rc;
  const int P = K + K * d;
  LoglikStage s;
  if (int rc = stage(h, [&](Layout& c) { s = loglik_stage(c, n, d, P, B); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, B, K, d, &dv)) return frc;
  // A small call (a speculative batch of Metropolis candidates, the points of a numerical derivative) is dominated by
  // the host side: through pageable memory every one of the three uploads and three downloads is a staged,
  // synchronous copy of its own.  Up to 1 MiB (inputs + results) the payload goes through the handle's pinned buffer:
  // ONE copy each way, the two spans of loglik_stage.
  const size_t pin_max = s.payload <= (size_t(1) << 20) ? kPinMax : 0;
  if (int prc = push(h, {piece(s.X, X, (size_t)n * d), piece(s.y, y, n), piece(s.params, params, (size_t)B * P)}, pin_max))
    return prc;
  if (int rc = loglik_run(h, s.X, n, d, s.y, dv, sigma2, mean_mode, tau2, s.loglik, s.beta, s.status)) return rc;
  return pull_status(h, {piece(s.loglik, out_loglik, B), piece(s.beta, out_beta, B)}, s.status, B, status, pin_max, true);
} CCGP_GUARD_END(h)

// ---- many training sets of one shape in one call (ccgp.h) -----------------------------------------------------------------
// what the sets entry points refuse before anything is copied or launched.  need_sigma2: the call reads a sigma2 per set;
// min_B: 1, or 0 where an empty call is legal
static bool sets_args_ok(const double* Xs, const double* ys, const double* sigma2, bool need_sigma2, int C, const int* set,
                         int B, int min_B) {
  if (C < 1 || B < min_B || !Xs || !ys || (need_sigma2 && !sigma2) || !set) return false;
  for (int b = 0; b < B; ++b)
    if (set[b] < 0 || set[b] >= C) return false;
  return true;
}

int ccgp_loglik_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                           int K, const double* params, const int* set, int B, int mean_mode, double tau2,
                           double* out_loglik, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || !params || !out_loglik || !sets_args_ok(Xs, ys, sigma2, true, C, set, B, 1))
    return fail(h, CCGP_EINVAL, "ccgp_loglik_batch_sets: bad argument");
  if (int rc = check_mean_mode(h, mean_mode)) return rc;
  const int P = K + K * d;
  if (small_route_sets(gauss_or_fused(h, n, d, K), n, d, K) == Route::Blocked) {   // ccgp_loglik_batch, whatever route that call takes
    std::vector<double> ll, beta;
    std::vector<int> st;
    return sets_by_group(set, B, C, P, params, [&](int c, const double* rows, int nb, const std::vector<int>& idx) -> int {
      ll.resize(nb); beta.resize(nb); st.resize(nb);
      const int rc = ccgp_loglik_batch(h, Xs + (size_t)c * n * d, n, d, ys + (size_t)c * n, K, rows, nb, sigma2[c], mean_mode,
                                       tau2, ll.data(), beta.data(), st.data());
      if (rc < 0) return rc;
      scatter_by(idx, ll, out_loglik);
      scatter_by(idx, beta, out_beta);
      scatter_by(idx, st, status);
      return rc;
    });
  }
  CCGP_HIP(hipSetDevice(h->device));
  SetsStage s;
  if (int rc = stage(h, [&](Layout& c) { s = sets_stage(c, n, d, P, C, B); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, B, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(Xs, ys, sigma2, params, set))) return prc;
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_loglik_sets(h->stream, s.Xs, n, d, s.ys, s.sigma2, s.set, dv, B, mean_mode, tau2, s.loglik, s.beta,
                                 s.status);
    CCGP_LAUNCH_CHECK();
  }
  return pull_status(h, s.results(out_loglik, out_beta), s.status, B, status);
} CCGP_GUARD_END(h)

int ccgp_loglik_grad_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                           const double* params, int B, double sigma2, double* out_loglik,
                           double* out_beta, double* out_grad, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 1 || !X || !y || !params || !out_grad)
    return fail(h, CCGP_EINVAL, "ccgp_loglik_grad_batch: bad argument");
  return grad_call(h, "ccgp_loglik_grad_batch", X, n, d, y, K, params, B, sigma2, out_loglik, nullptr, out_beta, out_grad, status);
} CCGP_GUARD_END(h)

// ---- ordinary-kriging MLE: the likelihood with sigma2 concentrated out (ccgp.h) -----------------------------------------
int ccgp_profile_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                       const double* params, int B, double* out_loglik, double* out_sigma2,
                       double* out_beta, double* out_grad, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 0 || !X || !y || !params || !out_loglik || !out_sigma2)
    return fail(h, CCGP_EINVAL, "ccgp_profile_batch: bad argument");
  if (B == 0) return CCGP_OK;
  return grad_call(h, "ccgp_profile_batch", X, n, d, y, K, params, B, 1.0, out_loglik, out_sigma2, out_beta, out_grad, status);
} CCGP_GUARD_END(h)

// ---- the CGP comparator of compare.GP (ccgp.h; kernels: cgp.hip) ---------------------------------------------------------
static int cgp_shape(ccgp_handle* h, const char* who, int n, int d) {
  if (!cgp_supported(n, d))
    return fail(h, CCGP_EUNSUPPORTED, std::string(who) + ": n must be <= 128 and the design must fit in LDS beside the "
                                      "working matrix (n = 128: d <= 21)");
  return CCGP_OK;
}

// ccgp_cgp_state_batch (set == nullptr: the one set of C = 1, launch_cgp_state) and ccgp_cgp_state_batch_sets behind their
// pointer checks: what both refuse before any launch, then the chunked call
static int cgp_state_call(ccgp_handle* h, const char* who, const double* Xs, int n, int d, const double* ys, int C,
                          const double* params, const int* set, int B, const int* skip, double* out_val, double* out_beta,
                          double* out_tau2, double* out_loo, int* status) {
  if (skip)
    for (int b = 0; b < B; ++b)
      if (skip[b] < -1 || skip[b] >= n || (skip[b] >= 0 && n < 2))
        return fail(h, CCGP_EINVAL, std::string(who) + ": skip must be -1 or a row of a design of at least two points");
  if (int rc = cgp_shape(h, who, n, d)) return rc;
  if (B == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = 2 * d + 2;
  return run_chunked(
      h, cgp_sets_row_bytes(d), params, B, P, nullptr, [&](Layout& w, int nb) { return cgp_sets_stage(w, n, d, C, nb); },
      [&](const CgpSetsStage& s, int b0, int nb, const double* rows, double*) -> int {
        // without `set` (the single-set call) or `skip` their staged words go up unwritten inside the one span; no kernel
        // reads them: launch_cgp_state takes no set array, and a null skip is passed on as null
        if (int prc = push(h, s.inputs(b0 == 0, Xs, ys, at(set, b0), at(skip, b0), rows, nb))) return prc;
        {
          ScopedTimer t(h, CCGP_T_FUSED);
          if (set)
            launch_cgp_state_sets(h->stream, s.Xs, n, d, s.ys, s.set, s.params, nb, nb, skip ? s.skip : nullptr, s.val, s.beta,
                                  s.tau2, out_loo ? s.loo : nullptr, s.status);
          else
            launch_cgp_state(h->stream, s.Xs, n, d, s.ys, s.params, nb, nb, skip ? s.skip : nullptr, s.val, s.beta, s.tau2,
                             out_loo ? s.loo : nullptr, s.status, nullptr);
        }
        CCGP_LAUNCH_CHECK();
        return pull_status(h, s.results(out_val + b0, at(out_beta, b0), at(out_tau2, b0), at(out_loo, b0), nb), s.status, nb,
                           at(status, b0));
      });
}

int ccgp_cgp_state_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, const double* params, int B,
                         const int* skip, double* out_val, double* out_beta, double* out_tau2, double* out_loo,
                         int* status) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || B < 0 || !X || !y || !params || !out_val)
    return fail(h, CCGP_EINVAL, "ccgp_cgp_state_batch: bad argument");
  return cgp_state_call(h, "ccgp_cgp_state_batch", X, n, d, y, 1, params, nullptr, B, skip, out_val, out_beta, out_tau2, out_loo,
                        status);
} CCGP_GUARD_END(h)

// ---- the comparator fits over many training sets of one shape (ccgp.h) ------------------------------------------------------
int ccgp_profile_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int K,
                            const double* params, const int* set, int B, double* out_loglik, double* out_sigma2,
                            double* out_beta, double* out_grad, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || !params || !out_loglik || !out_sigma2 || !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 0))
    return fail(h, CCGP_EINVAL, "ccgp_profile_batch_sets: bad argument");
  if (B == 0) return CCGP_OK;
  // (a 1-D family under CCGP_OPT_FAMILY_FUSED_GRAD counts as served, as in ccgp_profile_batch)
  const bool gauss = gauss_or_fused_grad(h, h->fam, n, d, K, out_grad != nullptr);
  // ccgp_profile_batch's refusals, before the first group is launched
  if (out_grad && !gauss)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_profile_batch_sets: analytic gradient is implemented for the Gaussian family only");
  if (out_grad && small_route(Op::Grad, gauss, n, d, K) == Route::Blocked && !blocked_grad_supported(d, K))
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_profile_batch_sets: d + K too large for the contraction kernel's LDS");
  const int P = K + K * d;
  if (!out_grad || small_route_profile_grad_sets(gauss, n, d, K) == Route::Blocked) {
    // no sets kernel for the call: ccgp_profile_batch per set, whatever route that call takes
    std::vector<double> ll, s2, beta, grad;
    std::vector<int> st;
    return sets_by_group(set, B, C, P, params, [&](int c, const double* rows, int nb, const std::vector<int>& idx) -> int {
      ll.resize(nb); s2.resize(nb); beta.resize(nb); st.resize(nb);
      if (out_grad) grad.resize((size_t)nb * P);
      const int rc = ccgp_profile_batch(h, Xs + (size_t)c * n * d, n, d, ys + (size_t)c * n, K, rows, nb, ll.data(), s2.data(),
                                        beta.data(), out_grad ? grad.data() : nullptr, st.data());
      if (rc < 0) return rc;
      scatter_by(idx, ll, out_loglik);
      scatter_by(idx, s2, out_sigma2);
      scatter_by(idx, beta, out_beta);
      scatter_by(idx, st, status);
      scatter_by(idx, grad, out_grad, P, B);
      return rc;
    });
  }
  CCGP_HIP(hipSetDevice(h->device));
  return run_chunked(
      h, profile_sets_row_bytes(P), params, B, P, out_grad,
      [&](Layout& w, int nb) { return profile_sets_stage(w, n, d, P, C, nb); },
      [&](const ProfileSetsStage& s, int b0, int nb, const double* rows, double* grad) -> int {
        DrawView dv;
        if (int frc = draw_view(h, h->fam, s.params, nb, K, d, &dv)) return frc;
        if (int prc = push(h, s.inputs(b0 == 0, Xs, ys, set + b0, rows, nb))) return prc;
        {
          ScopedTimer t(h, CCGP_T_FUSED);
          launch_small_reg_profile_grad_sets(h->stream, s.Xs, n, d, s.ys, s.set, dv, nb, s.loglik, s.s2hat, s.beta, s.grad,
                                             s.status);
        }
        CCGP_LAUNCH_CHECK();
        return pull_status(h, s.results(grad, out_loglik + b0, out_sigma2 + b0, at(out_beta, b0), nb), s.status, nb,
                           at(status, b0));
      });
} CCGP_GUARD_END(h)

int ccgp_cgp_state_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, const double* params,
                              const int* set, int B, const int* skip, double* out_val, double* out_beta, double* out_tau2,
                              double* out_loo, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || !params || !out_val || !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 0))
    return fail(h, CCGP_EINVAL, "ccgp_cgp_state_batch_sets: bad argument");
  return cgp_state_call(h, "ccgp_cgp_state_batch_sets", Xs, n, d, ys, C, params, set, B, skip, out_val, out_beta, out_tau2,
                        out_loo, status);
} CCGP_GUARD_END(h)

int ccgp_cgp_predict(ccgp_handle* h, const double* X, int n, int d, const double* y, const double* params,
                     const double* Xtest, int m, double* out, double* out_state, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || m < 0 || !X || !y || !params || (m > 0 && (!Xtest || !out)))
    return fail(h, CCGP_EINVAL, "ccgp_cgp_predict: bad argument");
  if (int rc = cgp_shape(h, "ccgp_cgp_predict", n, d)) return rc;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = 2 * d + 2;
  const CgpKeep kp(n);
  double *dX, *dy, *dp, *dXt, *dout, *dres, *dkeep;
  int* dst;
  auto lay = [&](Layout& w) {
    dX = w.take<double>((size_t)n * d);
    dy = w.take<double>(n);
    dp = w.take<double>(P);
    dXt = w.take<double>((size_t)m * d);
    dout = w.take<double>((size_t)m * 6);
    dres = w.take<double>(4);
    dst = w.take<int>(2);
    dkeep = w.take<double>(kp.total);
  };
  if (int rc = ensure(h, h->ws, kWorkspace, layout_bytes(lay))) return rc;
  Layout ws(h->ws.ptr);
  lay(ws);
  if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dy, y, n), piece(dp, params, P), piece(dXt, Xtest, (size_t)m * d)}))
    return prc;
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_cgp_state(h->stream, dX, n, d, dy, dp, 1, 1, nullptr, dres, dres + 1, dres + 2, nullptr, dst, dkeep);
    if (m > 0) launch_cgp_predict(h->stream, dX, n, d, dp, dXt, m, dkeep, dst, dout);
  }
  CCGP_LAUNCH_CHECK();
  int st = 0;
  const int rc = pull_status(h, {piece(dout, out, (size_t)m * 6), piece(dkeep + kp.s, out_state, (size_t)3 * n + 3)}, dst, 1, &st);
  if (rc < 0) return rc;
  if (status) *status = st;
  if (st && out_state)   // a failed state keeps nothing
    for (int i = 0; i < 3 * n + 3; ++i) out_state[i] = std::nan("");
  return rc;
} CCGP_GUARD_END(h)

// ccgp_cgp_predict over many training sets: one state launch and one site launch per chunk of rows, every row on its own kept
// block.  The sets, their responses and their test sites go up with the first chunk only.
int ccgp_cgp_predict_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, const double* params,
                          const int* set, int B, const double* Xtests, int m, double* out, double* out_state,
                          int* status) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || m < 0 || !params || (m > 0 && (!Xtests || !out)) ||
      !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 0))
    return fail(h, CCGP_EINVAL, "ccgp_cgp_predict_sets: bad argument");
  if (int rc = cgp_shape(h, "ccgp_cgp_predict_sets", n, d)) return rc;
  if (B == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = 2 * d + 2;
  const CgpKeep kp(n);
  const size_t ns = 3 * (size_t)n + 3;   // s | res2 | temp | sf, beta, tau2: contiguous in the kept block from kp.s on
  return run_chunked(
      h, cgp_predict_sets_row_bytes(n, d, m, kp.total), params, B, P, nullptr,
      [&](Layout& w, int nb) { return cgp_predict_sets_stage(w, n, d, C, m, kp.total, nb); },
      [&](const CgpPredictSetsStage& s, int b0, int nb, const double* rows, double*) -> int {
        if (int prc = push(h, s.inputs(b0 == 0, Xs, ys, Xtests, set + b0, rows, nb))) return prc;
        {
          ScopedTimer t(h, CCGP_T_FUSED);
          launch_cgp_state_sets_keep(h->stream, s.Xs, n, d, s.ys, s.set, s.params, nb, nb, s.res, s.res + nb,
                                     s.res + 2 * (size_t)nb, s.status, s.keep);
          if (m > 0)
            launch_cgp_predict_sets(h->stream, s.Xs, n, d, s.set, s.params, nb, nb, s.Xtests, m, s.keep, s.status, s.out);
        }
        CCGP_LAUNCH_CHECK();
        if (out_state)   // a failed row kept nothing: what is gathered for it is overwritten below
          CCGP_HIP(hipMemcpy2DAsync(s.state, sizeof(double) * ns, s.keep + kp.s, sizeof(double) * kp.total, sizeof(double) * ns,
                                    (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
        std::vector<int> st(nb);
        const int rc = pull_status(h, s.results(m > 0 ? out + (size_t)b0 * m * 6 : nullptr,
                                                out_state ? out_state + b0 * ns : nullptr, nb), s.status, nb, st.data());
        if (rc < 0) return rc;
        for (int r = 0; r < nb; ++r) {
          if (status) status[b0 + r] = st[r];
          if (st[r] && out_state)
            for (size_t i = 0; i < ns; ++i) out_state[(b0 + r) * ns + i] = std::nan("");
        }
        return rc;
      });
} CCGP_GUARD_END(h)

// ---- a8: logpost ------------------------------------------------------------------------------
// the argument checks ccgp_logpost and ccgp_logpost_batch share; `who` is the name the message carries
static int logpost_args(ccgp_handle* h, const char* who, bool shapes_ok, int d, int prior_id, const double* prior_pars) {
  auto bad = [&](const char* what) { return fail(h, CCGP_EINVAL, std::string(who) + what); };
  if (!shapes_ok) return bad(": bad argument");
  if (prior_id < CCGP_PRIOR_INVGAMMA || prior_id > CCGP_PRIOR_ANI) return bad(": unknown prior_id");
  if (prior_id == CCGP_PRIOR_INVGAMMA && !prior_pars) return bad(": prior_pars required for CCGP_PRIOR_INVGAMMA");
  if (prior_id == CCGP_PRIOR_ANI && d != 2) return bad(": the anisotropic script (ANI) is 2-D");
  return CCGP_OK;
}

int ccgp_logpost_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, double sigma2, int prior_id,
                       const double* theta_t, int B, const double* prior_pars, double* out_val, double* out_beta,
                       double* out_loglik, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (int rc = logpost_args(h, "ccgp_logpost_batch", n >= 1 && d >= 1 && d <= kMaxD && B >= 1 && X && y && theta_t && out_val,
                            d, prior_id, prior_pars))
    return rc;
  return logpost_rows(prior_id, d, theta_t, B, prior_pars, out_val, out_beta, out_loglik, status,
                      [&](int K, const double* rows, double* ll, double* beta, int* st) {
                        return ccgp_loglik_batch(h, X, n, d, y, K, rows, B, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, ll, beta, st);
                      });
} CCGP_GUARD_END(h)

// ccgp_logpost_batch over many training sets: the same host arithmetic around ccgp_loglik_batch_sets
int ccgp_logpost_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                      int prior_id, const double* theta_t, const int* set, int B, const double* prior_pars, double* out_val,
                      double* out_beta, double* out_loglik, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (int rc = logpost_args(h, "ccgp_logpost_sets",
                            n >= 1 && d >= 1 && d <= kMaxD && theta_t && out_val &&
                                sets_args_ok(Xs, ys, sigma2, true, C, set, B, 1),
                            d, prior_id, prior_pars))
    return rc;
  return logpost_rows(prior_id, d, theta_t, B, prior_pars, out_val, out_beta, out_loglik, status,
                      [&](int K, const double* rows, double* ll, double* beta, int* st) {
                        return ccgp_loglik_batch_sets(h, Xs, n, d, ys, sigma2, C, K, rows, set, B, CCGP_MEAN_PROFILE_BETA, 0.0,
                                                      ll, beta, st);
                      });
} CCGP_GUARD_END(h)

// ---- Metropolis chains on the device (ccgp.h) --------------------------------------------------------------------------------
int ccgp_chain_terms(int prior_id, int d, const double* theta_t, int B, const double* prior_pars, double* out_rows,
                     double* out_ljac, double* out_lprior) {
  if (d < 1 || d > kMaxD || B < 0 || !chain_prior_ok(prior_id, d, prior_pars) || !theta_t || !out_rows || !out_ljac || !out_lprior)
    return CCGP_EINVAL;
  try {
    chain_terms_rows(prior_id, d, theta_t, B, prior_pars, out_rows, out_ljac, out_lprior);
  } catch (...) {
    return CCGP_ENOMEM;
  }
  return CCGP_OK;
}

// the host twin of the chain kernel's evaluation: ccgp_logpost_sets with the portable terms in place of glibc's
int ccgp_chain_logpost_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                            int prior_id, const double* theta_t, const int* set, int B, const double* prior_pars,
                            double* out_val, double* out_beta, double* out_loglik, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (int rc = logpost_args(h, "ccgp_chain_logpost_sets",
                            n >= 1 && d >= 1 && d <= kMaxD && theta_t && out_val &&
                                sets_args_ok(Xs, ys, sigma2, true, C, set, B, 1),
                            d, prior_id, prior_pars))
    return rc;
  const int K = 2, P = K + K * d;
  std::vector<double> rows((size_t)B * P), ljac(B), lpri(B), ll(B), beta(B);
  std::vector<int> st(B);
  chain_terms_rows(prior_id, d, theta_t, B, prior_pars, rows.data(), ljac.data(), lpri.data());
  const int rc = ccgp_loglik_batch_sets(h, Xs, n, d, ys, sigma2, C, K, rows.data(), set, B, CCGP_MEAN_PROFILE_BETA, 0.0,
                                        ll.data(), beta.data(), st.data());
  if (rc < 0) return rc;
  for (int b = 0; b < B; ++b) {
    out_val[b] = chain_value(ll[b], ljac[b], lpri[b]);
    if (out_beta) out_beta[b] = beta[b];
    if (out_loglik) out_loglik[b] = ll[b];
    if (status) status[b] = st[b];
  }
  return rc;
} CCGP_GUARD_END(h)

int ccgp_metro_segments_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                             int prior_id, const double* prior_pars, int A, const int* set, const double* theta0,
                             const double* l0, const double* beta0, int T, const double* steps, const double* logu,
                             const int* n_prop, const int* stop_acc, int M, int* out_used, int* out_accepted,
                             double* out_draws, double* out_draw_val, double* out_draw_beta, double* out_theta, double* out_l,
                             double* out_beta, double* trace_val, double* trace_beta, int* trace_status,
                             int* trace_accept) try {
  if (!h) return CCGP_EINVAL;
  const int ntrace = (trace_val != nullptr) + (trace_beta != nullptr) + (trace_status != nullptr) + (trace_accept != nullptr);
  bool ok = n >= 1 && d >= 1 && d <= kMaxD && A >= 0 && T >= 1 && M >= 1 && theta0 && l0 && steps && logu && n_prop &&
            stop_acc && out_used && out_accepted && out_draws && out_draw_val && out_draw_beta && out_theta && out_l &&
            (ntrace == 0 || ntrace == 4) && sets_args_ok(Xs, ys, sigma2, true, C, set, A, 0);
  for (int a = 0; ok && a < A; ++a) ok = n_prop[a] >= 0 && n_prop[a] <= T && stop_acc[a] >= 0 && stop_acc[a] <= M;
  if (int rc = logpost_args(h, "ccgp_metro_segments_sets", ok, d, prior_id, prior_pars)) return rc;
  if (small_route_chain(gauss_or_fused(h, n, d, 2), n, d, 2) != Route::Reg)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_metro_segments_sets: chains run on the device for Gaussian sets of n <= 128 whose "
                                      "register-resident instance fits (the 1-D families: n <= 32 under CCGP_OPT_FAMILY_FUSED); "
                                      "keep the chain on ccgp_chain_logpost_sets");
  if (A == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const int q = prior_id == CCGP_PRIOR_ANI ? 4 : 3;
  const size_t sA = A, sT = (size_t)A * T, sM = (size_t)A * M;
  double *dXs, *dys, *ds2, *dpp, *dbeta0;
  int *dset, *dused;
  ChainIO io{};
  io.prior_id = prior_id; io.p = q; io.T = T; io.M = M;
  // inputs back to back, then results back to back: each side crosses PCIe as one span
  if (int rc = stage(h, [&](Layout& c) {
        dXs = c.take<double>((size_t)C * n * d);
        dys = c.take<double>((size_t)C * n);
        ds2 = c.take<double>(C);
        dpp = c.take<double>(4);
        io.prior_pars = dpp;
        io.theta0 = c.take<double>(sA * q);
        io.l0 = c.take<double>(sA);
        io.beta0 = dbeta0 = c.take<double>(sA);
        io.steps = c.take<double>(sT * q);
        io.logu = c.take<double>(sT);
        dset = c.take<int>(sA);
        io.n_prop = c.take<int>(sA);
        io.stop_acc = c.take<int>(sA);
        io.draws = c.take<double>(sM * q);
        io.draw_val = c.take<double>(sM);
        io.draw_beta = c.take<double>(sM);
        io.theta_fin = c.take<double>(sA * q);
        io.l_fin = c.take<double>(sA);
        io.beta_fin = c.take<double>(sA);
        io.used = dused = c.take<int>(3 * sA);   // used | accepted | failed
        io.nacc = dused ? dused + sA : nullptr;
        io.nfail = dused ? dused + 2 * sA : nullptr;
        io.tr_val = ntrace ? c.take<double>(sT) : nullptr;
        io.tr_beta = ntrace ? c.take<double>(sT) : nullptr;
        io.tr_status = ntrace ? c.take<int>(sT) : nullptr;
        io.tr_acc = ntrace ? c.take<int>(sT) : nullptr;
      }))
    return rc;
  const double kNaN = std::nan("");
  std::vector<double> b0(sA, kNaN);
  const double pp0[4] = {0.0, 0.0, 0.0, 0.0};
  if (int prc = push(h, {piece(dXs, Xs, (size_t)C * n * d), piece(dys, ys, (size_t)C * n), piece(ds2, sigma2, C),
                         piece(dpp, prior_pars ? prior_pars : pp0, 4), piece(const_cast<double*>(io.theta0), theta0, sA * q),
                         piece(const_cast<double*>(io.l0), l0, sA), piece(dbeta0, beta0 ? beta0 : b0.data(), sA),
                         piece(const_cast<double*>(io.steps), steps, sT * q), piece(const_cast<double*>(io.logu), logu, sT),
                         piece(dset, set, sA), piece(const_cast<int*>(io.n_prop), n_prop, sA),
                         piece(const_cast<int*>(io.stop_acc), stop_acc, sA)}))
    return prc;
  if (ntrace) {   // a chain that stops early leaves the rest of its trace as it is: NaN / -1, not what the buffer held
    CCGP_HIP(hipMemsetAsync(io.tr_val, 0xFF, Layout::al(sT * sizeof(double)) * 2 + Layout::al(sT * sizeof(int)) * 2, h->stream));
  }
  CCGP_HIP(hipMemsetAsync(io.draws, 0xFF, (size_t)((char*)io.theta_fin - (char*)io.draws), h->stream));
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_chain_sets(h->stream, dXs, n, d, dys, ds2, dset, A, io, h->fam);
    CCGP_LAUNCH_CHECK();
  }
  std::vector<int> cnt(3 * sA);
  if (int rc = pull(h, {piece(io.draws, out_draws, sM * q), piece(io.draw_val, out_draw_val, sM),
                        piece(io.draw_beta, out_draw_beta, sM), piece(io.theta_fin, out_theta, sA * q),
                        piece(io.l_fin, out_l, sA), piece(io.beta_fin, out_beta, out_beta ? sA : 0),
                        piece(dused, cnt.data(), 3 * sA), piece(io.tr_val, trace_val, ntrace ? sT : 0),
                        piece(io.tr_beta, trace_beta, ntrace ? sT : 0), piece(io.tr_status, trace_status, ntrace ? sT : 0),
                        piece(io.tr_acc, trace_accept, ntrace ? sT : 0)}))
    return rc;
  int failed = 0;
  for (int a = 0; a < A; ++a) {
    out_used[a] = cnt[a];
    out_accepted[a] = cnt[sA + a];
    failed += cnt[2 * sA + a];
  }
  return failed;
} CCGP_GUARD_END(h)

// ---- the ordinary-kriging fits on the device (ccgp.h) --------------------------------------------------------------------------
int ccgp_fit_state_doubles(int d) { return d >= 1 && d <= kMaxD ? fit_state_doubles(d) : CCGP_EINVAL; }

// what a state must say before anything steps it: the d it was begun with, a code and a pair count inside their ranges
static bool fit_state_ok(const double* st, int d) {
  return st[kFitD] == (double)d && st[kFitCode] >= 0.0 && st[kFitCode] <= (double)kFitNotEvaluable &&
         st[kFitCode] == (double)(int)st[kFitCode] && st[kFitPairs] >= 0.0 && st[kFitPairs] <= (double)kFitMemory &&
         st[kFitPairs] == (double)(int)st[kFitPairs];
}

int ccgp_fit_begin(double* state, int d, const double* x0, const double* lo, const double* hi, int maxit, double factr,
                   double pgtol, int max_backtracks) {
  if (d < 1 || d > kMaxD || !state || !x0 || !lo || !hi || maxit < 0 || max_backtracks < 0) return CCGP_EINVAL;
  fit_begin(state, d, x0, lo, hi, FitOpts{maxit, factr, pgtol, max_backtracks});
  return CCGP_OK;
}

int ccgp_fit_feed(double* state, int d, double f, const double* g, int ok) {
  if (d < 1 || d > kMaxD || !state || !g || !fit_state_ok(state, d)) return CCGP_EINVAL;
  fit_feed(state, f, g, ok != 0);
  return (int)state[kFitCode];
}

// the host twin of the fit kernel's evaluation: ccgp_profile_batch_sets on the rows (1, exp(logtheta)) with the portable exp
int ccgp_profile_fit_eval_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, const double* logtheta,
                               const int* set, int B, double* out_f, double* out_g, double* out_theta, double* out_sigma2,
                               double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, 1) || !logtheta || !out_f || !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 0))
    return fail(h, CCGP_EINVAL, "ccgp_profile_fit_eval_sets: bad argument");
  if (B == 0) return CCGP_OK;
  const ChainTables& tb = chain_tables();
  const int P = 1 + d;
  const size_t sB = B;
  std::vector<double> rows(sB * P), ll(sB), s2(sB), beta(sB), grad(out_g ? sB * P : 0);
  std::vector<int> st(sB);
  for (int b = 0; b < B; ++b) {
    rows[b] = 1.0;
    for (int k = 0; k < d; ++k) rows[b + (size_t)(1 + k) * sB] = fit_theta(logtheta[b + (size_t)k * sB], tb.hi, tb.lo);
  }
  const int rc = ccgp_profile_batch_sets(h, Xs, n, d, ys, C, 1, rows.data(), set, B, ll.data(), s2.data(), beta.data(),
                                         out_g ? grad.data() : nullptr, st.data());
  if (rc < 0) return rc;
  for (int b = 0; b < B; ++b) {
    out_f[b] = fit_value(ll[b]);
    if (out_sigma2) out_sigma2[b] = s2[b];
    if (out_beta) out_beta[b] = beta[b];
    if (status) status[b] = st[b];
    for (int k = 0; k < d; ++k) {
      const double th = rows[b + (size_t)(1 + k) * sB];
      if (out_theta) out_theta[b + (size_t)k * sB] = th;
      if (out_g) out_g[b + (size_t)k * sB] = fit_grad(grad[b + (size_t)(1 + k) * sB], th);
    }
  }
  return rc;
} CCGP_GUARD_END(h)

int ccgp_profile_fit_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int A, const int* set,
                          double* state, const int* max_evals, int* out_evals, double* trace_f, int* trace_status,
                          int T) try {
  if (!h) return CCGP_EINVAL;
  bool ok = !bad_shape(n, d, 1) && A >= 0 && T >= 0 && state && max_evals && out_evals &&
            (trace_f != nullptr) == (trace_status != nullptr) && sets_args_ok(Xs, ys, nullptr, false, C, set, A, 0);
  const int W = ok ? fit_state_doubles(d) : 0;
  const int cap = T < 4096 ? T : 4096;
  for (int a = 0; ok && a < A; ++a)
    ok = max_evals[a] >= 0 && max_evals[a] <= cap && fit_state_ok(state + (size_t)a * W, d);
  if (!ok) return fail(h, CCGP_EINVAL, "ccgp_profile_fit_sets: bad argument");
  if (small_route_fit(h->fam.id == 0, n, d, 1) != Route::Reg)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_profile_fit_sets: fits run on the device for Gaussian sets of n <= 128 whose "
                                      "register-resident gradient instance fits; keep the fit on ccgp_profile_fit_eval_sets");
  if (A == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const size_t sA = A, sT = (size_t)A * T;
  const bool tr = trace_f != nullptr && T > 0;
  double *dXs, *dys;
  int *dset, *dmax, *dcnt;
  FitIO io{};
  io.W = W; io.T = T;
  // inputs back to back, then results back to back: each side crosses PCIe as one span (the state is both)
  if (int rc = stage(h, [&](Layout& c) {
        dXs = c.take<double>((size_t)C * n * d);
        dys = c.take<double>((size_t)C * n);
        dset = c.take<int>(sA);
        dmax = c.take<int>(sA);
        io.state = c.take<double>(sA * W);
        dcnt = c.take<int>(2 * sA);   // evaluations | failed
        io.tr_f = tr ? c.take<double>(sT) : nullptr;
        io.tr_status = tr ? c.take<int>(sT) : nullptr;
      }))
    return rc;
  io.max_evals = dmax;
  io.evals = dcnt;
  io.nfail = dcnt ? dcnt + sA : nullptr;
  if (int prc = push(h, {piece(dXs, Xs, (size_t)C * n * d), piece(dys, ys, (size_t)C * n), piece(dset, set, sA),
                         piece(dmax, max_evals, sA), piece(io.state, state, sA * W)}))
    return prc;
  if (tr) {   // a start that stops early leaves the rest of its trace as it is: NaN / -1, not what the buffer held
    CCGP_HIP(hipMemsetAsync(io.tr_f, 0xFF, Layout::al(sT * sizeof(double)) + Layout::al(sT * sizeof(int)), h->stream));
  }
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_fit_sets(h->stream, dXs, n, d, dys, dset, A, io);
    CCGP_LAUNCH_CHECK();
  }
  std::vector<int> cnt(2 * sA);
  if (int rc = pull(h, {piece(io.state, state, sA * W), piece(dcnt, cnt.data(), 2 * sA), piece(io.tr_f, trace_f, tr ? sT : 0),
                        piece(io.tr_status, trace_status, tr ? sT : 0)}))
    return rc;
  int failed = 0;
  for (int a = 0; a < A; ++a) {
    out_evals[a] = cnt[a];
    failed += cnt[sA + a];
  }
  return failed;
} CCGP_GUARD_END(h)

// ---- the maximum-entropy design search on the device (ccgp.h) ----------------------------------------------------------------------
// the host twin of the design-search kernel's evaluation: ccgp_mixed_logdet_grad_designs on the designs (D_old on top of the
// free rows of block b of x), then f = -(ld - ld_offset), g = -grad in variable order
int ccgp_design_fit_eval(ccgp_handle* h, const double* D_old, int n_fixed, int n, int d, int K, const double* params,
                         double ld_offset, const double* x, int B, double* out_f, double* out_g, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || n_fixed < 0 || n_fixed >= n || (n_fixed > 0 && !D_old) || !params || B < 0 || !x || !out_f || !out_g)
    return fail(h, CCGP_EINVAL, "ccgp_design_fit_eval: bad argument");
  if (B == 0) return CCGP_OK;
  const int nfree = n - n_fixed;
  const size_t sB = B, nd = (size_t)n * d, nv = (size_t)nfree * d;
  std::vector<double> Xs(sB * nd), ld(sB), grad(sB * nv);
  std::vector<int> st(sB);
  for (size_t b = 0; b < sB; ++b)
    for (int k = 0; k < d; ++k) {
      double* col = Xs.data() + b * nd + (size_t)k * n;
      for (int i = 0; i < n_fixed; ++i) col[i] = D_old[i + (size_t)k * n_fixed];
      for (int i = 0; i < nfree; ++i) col[n_fixed + i] = x[b * nv + (size_t)i * d + k];
    }
  const int rc = ccgp_mixed_logdet_grad_designs(h, Xs.data(), n, d, B, K, params, n_fixed, ld.data(), grad.data(), st.data());
  if (rc < 0) return rc;
  for (size_t b = 0; b < sB; ++b) {
    out_f[b] = design_fit_value(ld[b], ld_offset);
    if (status) status[b] = st[b];
    for (int i = 0; i < nfree; ++i)
      for (int k = 0; k < d; ++k) out_g[b * nv + (size_t)i * d + k] = design_fit_grad(grad[b * nv + i + (size_t)k * nfree]);
  }
  return rc;
} CCGP_GUARD_END(h)

int ccgp_design_fit(ccgp_handle* h, const double* D_old, int n_fixed, int n, int d, int K, const double* params,
                    double ld_offset, int A, double* state, const int* max_evals, int* out_evals, double* trace_f,
                    int* trace_status, int T) try {
  if (!h) return CCGP_EINVAL;
  bool ok = !bad_shape(n, d, K) && n_fixed >= 0 && n_fixed < n && (n_fixed == 0 || D_old) && params && A >= 0 && T >= 0 &&
            state && max_evals && out_evals && (trace_f != nullptr) == (trace_status != nullptr);
  const long long nvl = ok ? (long long)(n - n_fixed) * d : 0;
  const bool steppable = nvl >= 1 && nvl <= kMaxD;   // beyond it no state exists to check: the route refuses below
  const int nv = steppable ? (int)nvl : 0, W = steppable ? fit_state_doubles(nv) : 0;
  const int cap = T < 4096 ? T : 4096;
  for (int a = 0; ok && a < A; ++a)
    ok = max_evals[a] >= 0 && max_evals[a] <= cap && (!steppable || fit_state_ok(state + (size_t)a * W, nv));
  if (!ok) return fail(h, CCGP_EINVAL, "ccgp_design_fit: bad argument");
  if (small_route_design_fit(h->fam.id == 0, n, d, K, n_fixed) != Route::Reg)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_design_fit: the search runs on the device for Gaussian designs of n <= 128 with at "
                                      "most 64 free coordinates whose design-gradient instance fits; keep it on "
                                      "ccgp_design_fit_eval");
  if (A == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  const size_t sA = A, sT = (size_t)A * T, nold = (size_t)n_fixed * d;
  const bool tr = trace_f != nullptr && T > 0;
  double *dold = nullptr, *dp;
  int *dmax, *dcnt;
  DesignFitIO io{};
  io.W = W; io.T = T; io.ld_offset = ld_offset;
  // inputs back to back, then results back to back: each side crosses PCIe as one span (the state is both)
  if (int rc = stage(h, [&](Layout& c) {
        dold = nold ? c.take<double>(nold) : nullptr;
        dp = c.take<double>(P);
        dmax = c.take<int>(sA);
        io.state = c.take<double>(sA * W);
        dcnt = c.take<int>(2 * sA);   // evaluations | failed
        io.tr_f = tr ? c.take<double>(sT) : nullptr;
        io.tr_status = tr ? c.take<int>(sT) : nullptr;
      }))
    return rc;
  io.D_old = dold;
  io.max_evals = dmax;
  io.evals = dcnt;
  io.nfail = dcnt ? dcnt + sA : nullptr;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
  if (int prc = push(h, {piece(dold, D_old, nold), piece(dp, params, P), piece(dmax, max_evals, sA),
                         piece(io.state, state, sA * W)}))
    return prc;
  if (tr) {   // a start that stops early leaves the rest of its trace as it is: NaN / -1, not what the buffer held
    CCGP_HIP(hipMemsetAsync(io.tr_f, 0xFF, Layout::al(sT * sizeof(double)) + Layout::al(sT * sizeof(int)), h->stream));
  }
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_design_fit(h->stream, n, d, dv, n_fixed, A, io);
    CCGP_LAUNCH_CHECK();
  }
  std::vector<int> cnt(2 * sA);
  if (int rc = pull(h, {piece(io.state, state, sA * W), piece(dcnt, cnt.data(), 2 * sA), piece(io.tr_f, trace_f, tr ? sT : 0),
                        piece(io.tr_status, trace_status, tr ? sT : 0)}))
    return rc;
  int failed = 0;
  for (int a = 0; a < A; ++a) {
    out_evals[a] = cnt[a];
    failed += cnt[sA + a];
  }
  return failed;
} CCGP_GUARD_END(h)

// ---- the CGP refinement on the device (ccgp.h) -----------------------------------------------------------------------------------
int ccgp_cgp_fit_rows(int d) { return d >= 1 && d <= (1 << 20) ? cgp_fit_rows(d) : CCGP_EINVAL; }

// the host twin of the refinement's evaluation: ccgp_cgp_state_batch_sets on the B R rows around the B points (cgp_fit_logic.h),
// then f = F_0, g_j from rows 1 + 2 j and 2 + 2 j, status = the centre row's
int ccgp_cgp_fit_eval_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, const double* w,
                           const double* lo, const double* hi, double step, const int* set, int B, double* out_f,
                           double* out_g, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || !w || !lo || !hi || !out_f || !out_g || !fit_finite(step) || !(step > 0.0) ||
      !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 0))
    return fail(h, CCGP_EINVAL, "ccgp_cgp_fit_eval_sets: bad argument");
  if (int rc = cgp_shape(h, "ccgp_cgp_fit_eval_sets", n, d)) return rc;
  if (B == 0) return CCGP_OK;
  const int P = cgp_fit_vars(d), R = cgp_fit_rows(d), NC = cgp_fit_cols(d);
  const size_t sB = B, nr = sB * R;
  if (nr > (size_t)0x7fffffff) return fail(h, CCGP_EUNSUPPORTED, "ccgp_cgp_fit_eval_sets: B (1 + 2 (d + 3)) rows exceed an int");
  std::vector<double> rows(nr * NC), val(nr), wv(P), lov(P), hiv(P);
  std::vector<int> row_set(nr), st(nr);
  for (size_t b = 0; b < sB; ++b) {
    for (int j = 0; j < P; ++j) {
      wv[j] = w[b + (size_t)j * sB];
      lov[j] = lo[b + (size_t)j * sB];
      hiv[j] = hi[b + (size_t)j * sB];
    }
    for (int r = 0; r < R; ++r) {
      row_set[b * R + r] = set[b];
      for (int c = 0; c < NC; ++c)
        rows[b * R + r + (size_t)c * nr] = cgp_fit_row_entry(wv.data(), lov.data(), hiv.data(), step, d, r, c);
    }
  }
  const int rc = ccgp_cgp_state_batch_sets(h, Xs, n, d, ys, C, rows.data(), row_set.data(), (int)nr, nullptr, val.data(), nullptr,
                                           nullptr, nullptr, st.data());
  if (rc < 0) return rc;
  int failed = 0;
  for (size_t b = 0; b < sB; ++b) {
    out_f[b] = cgp_fit_value(val[b * R]);
    if (status) status[b] = st[b * R];
    failed += st[b * R] != 0;
    for (int j = 0; j < P; ++j)
      out_g[b + (size_t)j * sB] = cgp_fit_grad(val[b * R + 1 + 2 * j], val[b * R + 2 + 2 * j], w[b + (size_t)j * sB], step,
                                               lo[b + (size_t)j * sB], hi[b + (size_t)j * sB]);
  }
  return failed;
} CCGP_GUARD_END(h)

int ccgp_cgp_fit_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int A, const int* set,
                      double* state, double step, const int* max_evals, int look, int* out_evals, double* trace_f,
                      int* trace_status, int T) try {
  if (!h) return CCGP_EINVAL;
  bool ok = n >= 1 && d >= 1 && A >= 0 && T >= 0 && look >= 1 && look <= 64 && fit_finite(step) && step > 0.0 &&
            state && max_evals && out_evals && (trace_f != nullptr) == (trace_status != nullptr) &&
            sets_args_ok(Xs, ys, nullptr, false, C, set, A, 0);
  const bool steppable = ok && d <= kMaxD - 3;   // beyond 64 variables no state exists to check: refused below
  const int P = steppable ? cgp_fit_vars(d) : 0, W = steppable ? fit_state_doubles(P) : 0;
  const int cap = T < 4096 ? T : 4096;
  int longest = 0;
  for (int a = 0; ok && a < A; ++a) {
    ok = max_evals[a] >= 0 && max_evals[a] <= cap && (!steppable || fit_state_ok(state + (size_t)a * W, P));
    longest = std::max(longest, max_evals[a]);
  }
  if (!ok) return fail(h, CCGP_EINVAL, "ccgp_cgp_fit_sets: bad argument");
  if (int rc = cgp_shape(h, "ccgp_cgp_fit_sets", n, d)) return rc;
  if (!steppable || (long long)A * cgp_fit_rows(d) > 65535)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_cgp_fit_sets: the refinement runs on the device for at most 64 variables and "
                                      "65535 rows per round; keep it on ccgp_cgp_fit_eval_sets");
  const int R = cgp_fit_rows(d), NC = cgp_fit_cols(d);
  const size_t sA = A, sT = (size_t)A * T, nr = sA * R;
  const bool tr = trace_f != nullptr && T > 0;
  double *dXs, *dys;
  int *dset, *dmax, *dcnt;
  CgpFitIO io{};
  io.W = W; io.T = T; io.step = step; io.ldp = (int)nr;
  // inputs back to back, then results back to back: each side crosses PCIe as one span (the state is both); behind them what
  // never leaves the device: gates, rows and the round's results
  auto lay = [&](Layout& c) {
    dXs = c.take<double>((size_t)C * n * d);
    dys = c.take<double>((size_t)C * n);
    dset = c.take<int>(sA);
    dmax = c.take<int>(sA);
    io.state = c.take<double>(sA * W);
    dcnt = c.take<int>(2 * sA);   // evaluations | centre rows failed
    io.tr_f = tr ? c.take<double>(sT) : nullptr;
    io.tr_status = tr ? c.take<int>(sT) : nullptr;
    io.gate = c.take<int>(sA);
    io.row_set = c.take<int>(nr);
    io.rows = c.take<double>(nr * NC);
    io.val = c.take<double>(nr);
    io.beta = c.take<double>(nr);
    io.tau2 = c.take<double>(nr);
    io.status = c.take<int>(nr);
  };
  if (layout_bytes(lay) > h->ws_limit)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_cgp_fit_sets: rows, results and states do not fit under the workspace limit in one "
                                      "piece; keep the refinement on ccgp_cgp_fit_eval_sets, whose call chunks");
  if (A == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  if (int rc = stage(h, lay)) return rc;
  io.set = dset;
  io.max_evals = dmax;
  io.evals = dcnt;
  io.nfail = dcnt + sA;
  if (int prc = push(h, {piece(dXs, Xs, (size_t)C * n * d), piece(dys, ys, (size_t)C * n), piece(dset, set, sA),
                         piece(dmax, max_evals, sA), piece(io.state, state, sA * W)}))
    return prc;
  if (tr) {   // a start that stops early leaves the rest of its trace as it is: NaN / -1, not what the buffer held
    CCGP_HIP(hipMemsetAsync(io.tr_f, 0xFF, Layout::al(sT * sizeof(double)) + Layout::al(sT * sizeof(int)), h->stream));
  }
  launch_cgp_fit_step(h->stream, d, A, io, true);
  CCGP_LAUNCH_CHECK();
  // `look` rounds of (gated evaluation, step) back to back, then the A gate words: the host looks only there.  A start makes
  // at most max_evals[a] evaluations, so `longest` rounds close every gate
  std::vector<int> gate(sA);
  for (int made = 0; made < longest;) {
    const int rounds = std::min(look, longest - made);
    {
      ScopedTimer t(h, CCGP_T_FUSED);
      for (int k = 0; k < rounds; ++k) {
        launch_cgp_state_gated(h->stream, dXs, n, d, dys, io, A);
        launch_cgp_fit_step(h->stream, d, A, io, false);
      }
      CCGP_LAUNCH_CHECK();
    }
    made += rounds;
    if (made >= longest) break;
    if (int rc = pull(h, {piece(io.gate, gate.data(), sA)})) return rc;
    if (std::none_of(gate.begin(), gate.end(), [](int g) { return g != 0; })) break;
  }
  std::vector<int> cnt(2 * sA);
  if (int rc = pull(h, {piece(io.state, state, sA * W), piece(dcnt, cnt.data(), 2 * sA), piece(io.tr_f, trace_f, tr ? sT : 0),
                        piece(io.tr_status, trace_status, tr ? sT : 0)}))
    return rc;
  int failed = 0;
  for (int a = 0; a < A; ++a) {
    out_evals[a] = cnt[a];
    failed += cnt[sA + a];
  }
  return failed;
} CCGP_GUARD_END(h)

// ---- the Laplace search on the device (ccgp.h) ----------------------------------------------------------------------------------
int ccgp_nm_state_doubles(int q) { return q >= 1 && q <= kNmMaxQ ? nm_state_doubles(q) : CCGP_EINVAL; }

// what a state must say before anything steps it: the q it was begun with, a code, a phase and a vertex inside their ranges
static bool nm_state_ok(const double* st, int q) {
  auto whole = [](double v, int lo, int hi) { return v >= (double)lo && v <= (double)hi && v == (double)(int)v; };
  return st[kNmQ] == (double)q && whole(st[kNmCode], kNmRunning, kNmMaxiter) &&
         whole(st[kNmPhase], kNmPhaseInit, kNmPhaseShrink) && whole(st[kNmVertex], 0, q);
}

int ccgp_nm_begin(double* state, int q, const double* x0, double xatol, double fatol, int maxiter) {
  if (q < 1 || q > kNmMaxQ || !state || !x0 || maxiter < 0) return CCGP_EINVAL;
  nm_begin(state, q, x0, xatol, fatol, maxiter);
  return CCGP_OK;
}

int ccgp_nm_feed(double* state, int q, double val) {
  if (q < 1 || q > kNmMaxQ || !state || !nm_state_ok(state, q)) return CCGP_EINVAL;
  nm_feed(state, val);
  return (int)state[kNmCode];
}

int ccgp_laplace_search_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                             int prior_id, const double* prior_pars, int A, const int* set, double* state,
                             const int* max_evals, int* out_evals, double* trace_val, int* trace_status, int T) try {
  if (!h) return CCGP_EINVAL;
  bool ok = n >= 1 && d >= 1 && d <= kMaxD && A >= 0 && T >= 0 && state && max_evals && out_evals &&
            (trace_val != nullptr) == (trace_status != nullptr) && sets_args_ok(Xs, ys, sigma2, true, C, set, A, 0);
  if (int rc = logpost_args(h, "ccgp_laplace_search_sets", ok, d, prior_id, prior_pars)) return rc;
  const int q = prior_id == CCGP_PRIOR_ANI ? 4 : 3, W = nm_state_doubles(q);
  const int cap = T < 4096 ? T : 4096;
  for (int a = 0; ok && a < A; ++a)
    ok = max_evals[a] >= 0 && max_evals[a] <= cap && nm_state_ok(state + (size_t)a * W, q);
  if (!ok) return fail(h, CCGP_EINVAL, "ccgp_laplace_search_sets: bad argument");
  if (small_route_nm(gauss_or_fused(h, n, d, 2), n, d, 2) != Route::Reg)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_laplace_search_sets: searches run on the device for Gaussian sets of n <= 128 whose "
                                      "register-resident instance fits (the 1-D families: n <= 32 under CCGP_OPT_FAMILY_FUSED); "
                                      "keep the search on ccgp_chain_logpost_sets and ccgp_nm_feed");
  if (A == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  const size_t sA = A, sT = (size_t)A * T;
  const bool tr = trace_val != nullptr && T > 0;
  double *dXs, *dys, *ds2, *dpp;
  int *dset, *dmax, *dcnt;
  NmIO io{};
  io.prior_id = prior_id; io.q = q; io.W = W; io.T = T;
  // inputs back to back, then results back to back: each side crosses PCIe as one span (the state is both)
  if (int rc = stage(h, [&](Layout& c) {
        dXs = c.take<double>((size_t)C * n * d);
        dys = c.take<double>((size_t)C * n);
        ds2 = c.take<double>(C);
        dpp = c.take<double>(4);
        dset = c.take<int>(sA);
        dmax = c.take<int>(sA);
        io.state = c.take<double>(sA * W);
        dcnt = c.take<int>(2 * sA);   // evaluations | failed
        io.tr_val = tr ? c.take<double>(sT) : nullptr;
        io.tr_status = tr ? c.take<int>(sT) : nullptr;
      }))
    return rc;
  io.prior_pars = dpp;
  io.max_evals = dmax;
  io.evals = dcnt;
  io.nfail = dcnt ? dcnt + sA : nullptr;
  const double pp0[4] = {0.0, 0.0, 0.0, 0.0};
  if (int prc = push(h, {piece(dXs, Xs, (size_t)C * n * d), piece(dys, ys, (size_t)C * n), piece(ds2, sigma2, C),
                         piece(dpp, prior_pars ? prior_pars : pp0, 4), piece(dset, set, sA), piece(dmax, max_evals, sA),
                         piece(io.state, state, sA * W)}))
    return prc;
  if (tr) {   // a search that stops early leaves the rest of its trace as it is: NaN / -1, not what the buffer held
    CCGP_HIP(hipMemsetAsync(io.tr_val, 0xFF, Layout::al(sT * sizeof(double)) + Layout::al(sT * sizeof(int)), h->stream));
  }
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_nm_sets(h->stream, dXs, n, d, dys, ds2, dset, A, io, h->fam);
    CCGP_LAUNCH_CHECK();
  }
  std::vector<int> cnt(2 * sA);
  if (int rc = pull(h, {piece(io.state, state, sA * W), piece(dcnt, cnt.data(), 2 * sA), piece(io.tr_val, trace_val, tr ? sT : 0),
                        piece(io.tr_status, trace_status, tr ? sT : 0)}))
    return rc;
  int failed = 0;
  for (int a = 0; a < A; ++a) {
    out_evals[a] = cnt[a];
    failed += cnt[sA + a];
  }
  return failed;
} CCGP_GUARD_END(h)

int ccgp_logpost(ccgp_handle* h, const double* X, int n, int d, const double* y, double sigma2,
                 int prior_id, const double* theta_t, const double* prior_pars, double* out_val,
                 double* out_beta, double* out_loglik, double* out_Rinv, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (int rc = logpost_args(h, "ccgp_logpost", n >= 1 && d >= 1 && d <= kMaxD && X && y && theta_t && out_val, d, prior_id,
                            prior_pars))
    return rc;
  const int K = 2, P = K + K * d;
  std::vector<double> row(P);
  double log_jacob = 0.0, log_prior = 0.0;
  logpost_terms(prior_id, d, theta_t, 1, prior_pars, row.data(), 1, &log_jacob, &log_prior);
  // ONE factorisation per call (the reference runs two: solve(R) at HX:454 and the Cholesky inside dmnorm at
  // HX:460): without R.Inv the batched evaluator; with it, a sweep that carries y', 1' AND the identity rows,
  // so the likelihood, beta and R^-1 come out of the same elimination
  double ll = 0.0, beta = 0.0;
  int st = 0;
  CCGP_HIP(hipSetDevice(h->device));
  const bool gauss = h->fam.id == 0;
  Route route = out_Rinv ? small_route(Op::Inverse, gauss, n, d, K) : small_route(Op::Loglik, gauss_or_fused(h, n, d, K), n, d, K);
  const size_t in_d = (size_t)n * d + n + P;                       // X | y | row
  const size_t out_d = 3 + (out_Rinv ? (size_t)n * n : 0);         // ll, beta, status (as one double slot) | R^-1
  if (route == Route::Reg && ensure(h, h->pin, kPinned, sizeof(double) * (in_d + out_d)) == CCGP_OK) {
    // The sequential caller's path (Metro evaluates ONE proposal per logpost call, HX:505-512): latency, not
    // throughput.  Inputs are packed into a pinned host buffer and cross PCIe in ONE copy, the results (log-lik,
    // beta, status[, R^-1]) come back in one: 300 -> ~100 us per call with R.Inv at n = 64, 113 -> ~60 us without (round 2).
    // With R.Inv the kernel stores its results STRAIGHT into the pinned host buffer (device-visible like any hipHostMalloc
    // memory): no device-to-host copy of the n x n inverse behind the kernel -- 84 -> 72 us per call at n = 64, 125 -> 115 at
    // n = 90.  (Value only: three doubles, no difference; reading the INPUTS through PCIe from the kernel is slower.)
    const bool zo = out_Rinv != nullptr;
    double *din, *dout = nullptr;
    if (int rc2 = stage(h, [&](Layout& c) {
          din = c.take<double>(in_d);
          if (!zo) dout = c.take<double>(out_d);
        }))
      return rc2;
    double* pout = static_cast<double*>(h->pin.ptr) + in_d;
    if (zo) dout = pout;
    double* dX = din;
    double* dy = din + (size_t)n * d;
    double* dp = dy + n;
    int* dst = reinterpret_cast<int*>(dout + 2);
    DrawView dv;
    if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
    if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dy, y, n), piece(dp, row.data(), P)})) return prc;
    {
      ScopedTimer t(h, CCGP_T_FUSED);
      if (out_Rinv)
        launch_small_reg_inverse(h->stream, dX, n, d, dy, dv, 0, sigma2, dout + 3, dout, dout + 1, dst);
      else
        launch_small_reg_loglik(h->stream, dX, n, d, dy, dv, 1, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, dout, dout + 1, dst);
    }
    CCGP_LAUNCH_CHECK();
    if (!zo) CCGP_HIP(hipMemcpyAsync(pout, dout, sizeof(double) * out_d, hipMemcpyDeviceToHost, h->stream));
    CCGP_HIP(hipStreamSynchronize(h->stream));
    ll = pout[0];
    beta = pout[1];
    std::memcpy(&st, pout + 2, sizeof(int));
    if (out_Rinv) std::memcpy(out_Rinv, pout + 3, sizeof(double) * (size_t)n * n);
  } else if (!out_Rinv) {
    int rc = ccgp_loglik_batch(h, X, n, d, y, K, row.data(), 1, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, &ll, &beta,
                               &st);
    if (rc < 0) return rc;
  } else {
    if (route == Route::Reg) route = small_route_inverse_staged(gauss, n, d);   // no pinned buffer
    double *dX, *dy, *dp, *dR, *dll, *dbt;
    int* dst;
    if (int rc2 = stage(h, [&](Layout& c) {
          dX = c.take<double>((size_t)n * d);
          dy = c.take<double>(n);
          dp = c.take<double>(P);
          dR = c.take<double>((size_t)n * n);
          dll = c.take<double>(1);
          dbt = c.take<double>(1);
          dst = c.take<int>(1);
        }))
      return rc2;
    DrawView dv;
    if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
    if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dy, y, n), piece(dp, row.data(), P)})) return prc;
    if (route == Route::Blocked) {
      // identity as extra tile rows of the blocked sweep, then R^-1 = Z Z' tile by tile
      BlockedJob job{};
      job.kind = kJobInverse; job.Rinv = dR;
      if (int rc2 = run_sweep(h, dX, n, d, dy, dv, 1, round_up(n, kTile) / kTile, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0,
                              {dll, dbt, dst}, &job, 0, no_scratch))
        return rc2;
    } else {
      CCGP_HIP(hipMemsetAsync(dst, 0, sizeof(int), h->stream));
      ScopedTimer t(h, CCGP_T_FUSED);
      launch_small_inverse(h->stream, dX, n, d, dy, dv, 0, sigma2, dR, dll, dbt, dst);
      CCGP_LAUNCH_CHECK();
    }
    if (int rc2 = pull_status(h, {piece(dR, out_Rinv, (size_t)n * n), piece(dll, &ll, 1), piece(dbt, &beta, 1)}, dst, 1, &st);
        rc2 < 0)
      return rc2;
  }
  *out_val = ll + log_jacob + log_prior;
  if (out_beta) *out_beta = beta;
  if (out_loglik) *out_loglik = ll;
  if (status) *status = st;
  return st != 0 ? 1 : 0;
} CCGP_GUARD_END(h)

// ---- 8(f)-4: entropy criteria over candidate designs ------------------------------------------------
int ccgp_mixed_logdet_designs(ccgp_handle* h, const double* Xs, int n, int d, int B, int K,
                              const double* params, double* out_logdet, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 1 || !Xs || !params || !out_logdet)
    return fail(h, CCGP_EINVAL, "ccgp_mixed_logdet_designs: bad argument");
  if (h->fam.id != 0)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_mixed_logdet_designs: Gaussian family only (BSQ:856-877)");
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  // more than 128 points (or too wide for the register-resident evaluator): the blocked sweep, one design at a time --
  // its chunk shares ONE design among its matrices, and here every matrix has its own.  The reference's candidate
  // sets are small (BSQ:856-877: a few dozen points); this branch exists so that the entry point has no size limit.
  const bool blocked = small_route(Op::LogdetDesigns, true, n, d, K) == Route::Blocked;
  const int npad = round_up(n, kTile);
  double *dXs, *dp, *dld, *dy = nullptr, *dll = nullptr, *dbeta = nullptr;
  int* dst;
  if (int rc = stage(h, [&](Layout& c) {
        dXs = c.take<double>((size_t)B * n * d);
        if (blocked) dy = c.take<double>(n);   // the sweep carries a right-hand side: zeros
        dp = c.take<double>(P);
        dld = c.take<double>(B);
        if (blocked) dll = c.take<double>(B);
        if (blocked) dbeta = c.take<double>(B);
        dst = c.take<int>(B);
      }))
    return rc;
  if (int rc = blocked ? ensure(h, h->ws, kWorkspace, blocked_ws_bytes(npad, 1, 0) + 512) : CCGP_OK) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
  if (int prc = push(h, {piece(dXs, Xs, (size_t)B * n * d), piece(dp, params, P)})) return prc;
  if (blocked) {
    CCGP_HIP(hipMemsetAsync(dy, 0, sizeof(double) * n, h->stream));
    CCGP_HIP(hipMemsetAsync(dst, 0, sizeof(int) * (size_t)B, h->stream));
    BlockedWs w = blocked_carve(h->ws.ptr, npad, 1, 0);
    for (int i = 0; i < B; ++i) {
      BlockedJob job{};
      job.kind = kJobLogdet;
      job.logdet = dld + i;
      blocked_loglik(h, dXs + (size_t)i * n * d, n, d, dy, dv, 0, 1, npad, 1.0, CCGP_MEAN_PROFILE_BETA, 0.0, w, dll + i,
                     dbeta + i, dst + i, &job);
    }
  } else {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_logdet_designs(h->stream, dXs, n, d, dv, B, dld, dst);
  }
  CCGP_LAUNCH_CHECK();
  return pull_status(h, {piece(dld, out_logdet, B)}, dst, B, status);
} CCGP_GUARD_END(h)

// d log det R_mixed / d X for B candidate designs (BSQ:856-948: the design search of Entropy.optim / Batch.Entropy.optim)
int ccgp_mixed_logdet_grad_designs(ccgp_handle* h, const double* Xs, int n, int d, int B, int K,
                                   const double* params, int n_fixed, double* out_logdet, double* out_grad,
                                   int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 1 || !Xs || !params || !out_logdet || !out_grad)
    return fail(h, CCGP_EINVAL, "ccgp_mixed_logdet_grad_designs: bad argument");
  if (n_fixed < 0 || n_fixed >= n)
    return fail(h, CCGP_EINVAL, "ccgp_mixed_logdet_grad_designs: n_fixed must lie in [0, n)");
  if (h->fam.id != 0)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_mixed_logdet_grad_designs: Gaussian family only (BSQ:856-948)");
  if (small_route(Op::DesignGrad, true, n, d, K) == Route::Unsupported)
    return fail(h, CCGP_EUNSUPPORTED, "ccgp_mixed_logdet_grad_designs: the design does not fit the register-resident "
                                      "evaluator (n <= 128 and its LDS share: R^-1 and the design of one matrix)");
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  const size_t ng = (size_t)B * (n - n_fixed) * d;
  double *dXs, *dp, *dld, *dg;
  int* dst;
  if (int rc = stage(h, [&](Layout& c) {
        dXs = c.take<double>((size_t)B * n * d);
        dp = c.take<double>(P);
        dld = c.take<double>(B);
        dg = c.take<double>(ng);
        dst = c.take<int>(B);
      }))
    return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dp, 1, K, d, &dv)) return frc;
  if (int prc = push(h, {piece(dXs, Xs, (size_t)B * n * d), piece(dp, params, P)})) return prc;
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_logdet_grad_designs(h->stream, dXs, n, d, dv, B, n_fixed, dld, dg, dst);
  }
  CCGP_LAUNCH_CHECK();
  return pull_status(h, {piece(dld, out_logdet, B), piece(dg, out_grad, ng)}, dst, B, status);
} CCGP_GUARD_END(h)

// ---- a9: hyperprior grid ------------------------------------------------------------------------
int ccgp_halton_base2(int N, double* out) {
  if (N < 0 || !out) return CCGP_EINVAL;
  halton_base2(N, out);
  return CCGP_OK;
}

int ccgp_qigamma(const double* p, int N, double alpha, double beta, double* out) {
  if (N < 0 || !p || !out || !(alpha > 0.0) || !(beta > 0.0)) return CCGP_EINVAL;
  for (int i = 0; i < N; ++i) out[i] = qigamma_host(p[i], alpha, beta);
  return CCGP_OK;
}

int ccgp_grid_marginal(ccgp_handle* h, const double* X, int n, int d, const double* y,
                       double sigma2, const double* hyper, int G, int N, double tau, int take_log,
                       double aniso_lambda, double* out, int* out_argmax, double* out_logs) try {
  if (!h) return CCGP_EINVAL;
  if (n < 1 || d < 1 || d > kMaxD || G < 1 || N < 1 || !X || !y || !hyper || !out)
    return fail(h, CCGP_EINVAL, "ccgp_grid_marginal: bad argument");
  const bool aniso = aniso_lambda >= 0.0;
  if (aniso && d != 2) return fail(h, CCGP_EINVAL, "ccgp_grid_marginal: anisotropic kernel is 2-D");
  CCGP_HIP(hipSetDevice(h->device));
  const int K = 2, P = K + K * d;
  const size_t B = (size_t)G * N;
  if (B > (size_t)1 << 30) return fail(h, CCGP_EINVAL, "ccgp_grid_marginal: G*N too large");
  // What crosses PCIe: X, y, the G x 4 hyperparameter matrix and the list of DISTINCT inverse-gamma shapes
  // (a few KB) in; G doubles and one failure count out.  The G x N table of draws is built in HBM:
  // unit-rate gamma quantiles per distinct shape (grid_qtab_kernel; the same Halton node drives p, theta1 and
  // theta2, HX:554-556), then the parameter rows (grid_expand_kernel).
  std::vector<double> shapes;
  std::vector<int> shape_idx(2 * (size_t)G);
  {
    std::map<double, int> seen;
    for (int g = 0; g < G; ++g) {
      const double a1 = hyper[g], b1 = hyper[g + (size_t)G], a2 = hyper[g + (size_t)2 * G],
                   b2 = hyper[g + (size_t)3 * G];
      if (!(a1 > 0.0) || !(b1 > 0.0) || !(a2 > 0.0) || !(b2 > 0.0))
        return fail(h, CCGP_EINVAL, "ccgp_grid_marginal: hyperparameters must be positive");
      for (int w = 0; w < 2; ++w) {
        const double al = w ? a2 : a1;
        auto it = seen.find(al);
        if (it == seen.end()) {
          it = seen.emplace(al, (int)shapes.size()).first;
          shapes.push_back(al);
        }
        shape_idx[(size_t)w * G + g] = it->second;
      }
    }
  }
  const size_t ns = shapes.size();
  double *dX, *dy, *dhy, *dsh, *dq, *dp, *dll, *dbeta, *dout;
  int *dsi, *dst, *dbad;
  if (int rc = stage(h, [&](Layout& c) {
        dX = c.take<double>((size_t)n * d);
        dy = c.take<double>(n);
        dhy = c.take<double>((size_t)4 * G);
        dsh = c.take<double>(ns);
        dsi = c.take<int>((size_t)2 * G);
        dq = c.take<double>(ns * N);
        dp = c.take<double>(B * P);
        dbeta = c.take<double>(B);
        dst = c.take<int>(B);
        dll = c.take<double>(B);   // the results close the buffer, logs | out | bad: one span down with out_logs or without
        dout = c.take<double>(G);
        dbad = c.take<int>(1);
      }))
    return rc;
  if (int prc = push(h, {piece(dX, X, (size_t)n * d), piece(dy, y, n), piece(dhy, hyper, (size_t)4 * G),
                         piece(dsh, shapes.data(), ns), piece(dsi, shape_idx.data(), (size_t)2 * G)}))
    return prc;
  CCGP_HIP(hipMemsetAsync(dbad, 0, sizeof(int), h->stream));
  {
    ScopedTimer t(h, CCGP_T_COV);
    // ns x N quantiles (a dozen shapes x 1000 nodes: ~12 000 threads, each a long serial Halley iteration) cannot fill
    // the chip; what matters is each wave's own speed.  One wave per workgroup spreads them over ~190 CUs where a lone
    // wave issues every 7.5 cycles, against one instruction per ~19 cycles when four waves share a SIMD
    // (profiles/r04/valu_f64_rates.txt): 1.96 -> 1.17 ms of the Heat-Exchanger grid's 11 ms end to end (and 0.08 once the quantile iteration stops at rounding level: special_math.h)
    hipLaunchKernelGGL(grid_qtab_kernel, dim3((unsigned)((ns * N + 63) / 64)), dim3(64), 0, h->stream, dsh, (int)ns, N, dq);
    hipLaunchKernelGGL(grid_expand_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, dhy, dsi, dq, G, N,
                       d, aniso ? 1 : 0, aniso_lambda, dp);
  }
  if (int rc = loglik_dev(h, dX, n, d, dy, K, dp, (int)B, sigma2, CCGP_MEAN_ZERO_PLUS_TAU2, tau * tau, dll, dbeta, dst))
    return rc;
  hipLaunchKernelGGL(row_logmeanexp_kernel, dim3(G), dim3(256), 0, h->stream, dll, N, take_log, dout);
  hipLaunchKernelGGL(count_bad_kernel, dim3((unsigned)((B + 1023) / 1024)), dim3(256), 0, h->stream, dst, (int)B, dbad);
  CCGP_LAUNCH_CHECK();
  int bad = 0;
  if (int rc = pull(h, {piece(dll, out_logs, B), piece(dout, out, G), piece(dbad, &bad, 1)})) return rc;
  if (out_argmax) {
    // which.max: first maximum, NaN skipped
    int best = -1;
    for (int g = 0; g < G; ++g)
      if (out[g] == out[g] && (best < 0 || out[g] > out[best])) best = g;
    *out_argmax = best;
  }
  return bad;
} CCGP_GUARD_END(h)

// ---- a10/a11: prediction -------------------------------------------------------------------------
// the prediction of the S draws of dv (kernel family included) at m test sites, on resident inputs; arguments are
// checked by the callers
static int predict_run(ccgp_handle* h, const double* dX, int n, int d, const double* dy, const DrawView& dv,
                       const double* dXtest, int m, double sigma2, double* d_mean, double* d_var, double* d_beta,
                       int* d_status, VarForm vf = VarForm{}) {
  const int K = dv.K, S = dv.ldp;
  // a 1-D family under CCGP_OPT_FAMILY_FUSED_PREDICT has the kept-factor scheme and nothing else (no FAM instance carries
  // extra rows): its scratch is secured BEFORE the route is taken, and without it the call is the sweep's
  const bool family = dv.fam.id != 0;
  bool gauss = gauss_or_fused_predict(h, dv.fam, n, d, K);
  void* scratch = nullptr;
  size_t sbytes = 0;
  if (family && gauss) {
    const size_t want = kept_factor_ws_bytes(h, gauss, n, d, K, S, m);
    if (want && ensure(h, h->ws, kWorkspace, want) == CCGP_OK && h->ws.bytes >= small_reg_sites_scratch(n, d, K, m)) {
      scratch = h->ws.ptr; sbytes = h->ws.bytes;
    } else {
      gauss = false;
    }
  }
  if (small_route(Op::Predict, gauss, n, d, K) == Route::Blocked) {
    // the m cross-correlation rows ride along as extra tile rows of the sweep; scratch for the outputs the caller did not
    // ask for lives behind the matrices
    SweepOut sc{};
    BlockedJob pr{};
    pr.kind = kJobPredict; pr.Xtest = dXtest; pr.m = m; pr.S = S; pr.mean = d_mean; pr.var = d_var; pr.vf = vf;
    return run_sweep(h, dX, n, d, dy, dv, S, (m + kTile - 1) / kTile, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, sc, &pr, 0,
                     [&](Layout& t, int) { sc = predict_tail(t, S, d_beta, d_status); });
  }
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    // kept-factor scheme where it applies (n <= 104, K <= 3) and its scratch fits the workspace.  After ccgp_reserve of
    // this shape both steps find what they need; a caller that never reserved pays for them here, once.
    if (!family) {
      if (const size_t want = kept_factor_ws_bytes(h, true, n, d, K, S, m))
        if (ensure(h, h->ws, kWorkspace, want) == CCGP_OK) { scratch = h->ws.ptr; sbytes = h->ws.bytes; }
    }
    if (scratch) (void)ensure_aux(h);
    launch_small_reg_predict(h->stream, dX, n, d, dy, dv, S, dXtest, m, sigma2, d_mean, d_var, d_beta,
                             d_status, scratch, sbytes, h->aux_stream, h->aux_fork, h->aux_join, vf);
  }
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}

int ccgp_predict_batch_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                           const double* dparams, int S, const double* dXtest, int m,
                           double sigma2, double* d_mean, double* d_var, double* d_beta,
                           int* d_status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || S < 1 || m < 1 || !dX || !dy || !dparams || !dXtest || !d_mean || !d_var)
    return fail(h, CCGP_EINVAL, "ccgp_predict_batch: bad argument");
  CCGP_HIP(hipSetDevice(h->device));
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dparams, S, K, d, &dv)) return frc;
  return predict_run(h, dX, n, d, dy, dv, dXtest, m, sigma2, d_mean, d_var, d_beta, d_status);
} CCGP_GUARD_END(h)

// ccgp_predict_batch and, with `krige`, ccgp_krige_predict_batch behind their argument checks.  krige: the
// staging carries the per-row tail, sigma2_row (nullptr: CCGP_VAR_UNBIASED reads none) goes up with the inputs and Q comes
// back with the results; the scalar is not read where the per-row pointer is set.
static int predict_call(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                        const double* params, int S, const double* Xtest, int m, double sigma2, bool krige,
                        const double* sigma2_row, int var_form, double* out_mean, double* out_var, double* out_beta,
                        double* out_q, int* status) {
  CCGP_HIP(hipSetDevice(h->device));
  PredictStage s;
  if (int rc = stage(h, [&](Layout& c) { s = predict_stage(c, n, d, K + K * d, S, m, krige); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.in.params, S, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(X, y, params, Xtest, sigma2_row))) return prc;
  const VarForm vf = krige ? VarForm{sigma2_row ? s.sigma2 : nullptr, var_form, s.q} : VarForm{};
  if (int rc = predict_run(h, s.in.X, n, d, s.in.y, dv, s.in.Xtest, m, sigma2, s.mean, s.var, s.beta, s.status, vf)) return rc;
  return pull_status(h, s.results(out_mean, out_var, out_beta, out_q), s.status, S, status);
}

int ccgp_predict_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                       const double* params, int S, const double* Xtest, int m, double sigma2,
                       double* out_mean, double* out_var, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || S < 1 || m < 1 || !X || !y || !params || !Xtest || !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_predict_batch: bad argument");
  return predict_call(h, X, n, d, y, K, params, S, Xtest, m, sigma2, false, nullptr, 0, out_mean, out_var,
                      out_beta, nullptr, status);
} CCGP_GUARD_END(h)

// ---- the single-GP comparator's prediction: ccgp_predict_batch's route with a per-row sigma2 and a variance form ---------
int ccgp_krige_predict_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                             const double* params, int B, const double* sigma2, int var_form, const double* Xtest, int m,
                             double* out_mean, double* out_var, double* out_beta, double* out_q, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 1 || m < 1 || !X || !y || !params || !Xtest || !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch: bad argument");
  if (var_form != CCGP_VAR_ORDINARY && var_form != CCGP_VAR_PLUGIN && var_form != CCGP_VAR_UNBIASED)
    return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch: unknown var_form");
  const bool own_s2 = var_form != CCGP_VAR_UNBIASED;
  if (!own_s2 && n < 2) return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch: CCGP_VAR_UNBIASED divides by n - 1");
  if (own_s2) {
    if (!sigma2) return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch: this var_form needs sigma2");
    for (int b = 0; b < B; ++b)
      if (!(std::isfinite(sigma2[b]) && sigma2[b] >= 0.0))
        return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch: every sigma2 must be finite and >= 0");
  }
  return predict_call(h, X, n, d, y, K, params, B, Xtest, m, 1.0, true, own_s2 ? sigma2 : nullptr,
                      var_form, out_mean, out_var, out_beta, out_q, status);
} CCGP_GUARD_END(h)

// ---- prediction(): per-site summaries of the tables, HX:686-703 / GV:620-638 -------------------------------------
int ccgp_predict_summary_dev(ccgp_handle* h, const double* dX, int n, int d, const double* dy, int K,
                             const double* dparams, int S, const double* dXtest, int m, double sigma2,
                             const double* probs, int n_probs, const double* d_y_at, double* d_out,
                             double* d_beta, int* d_status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || S < 1 || !dX || !dy || !dparams || !dXtest || !d_out)
    return fail(h, CCGP_EINVAL, "ccgp_predict_summary: bad argument");
  if (int rc = check_summary_args(h, m, probs, n_probs)) return rc;
  CCGP_HIP(hipSetDevice(h->device));
  SummaryDevStage sd;
  if (int rc = stage(h, [&](Layout& c) { sd = summary_dev_stage(c, S, m, !d_status); })) return rc;
  const SummaryTables& t = sd.t;
  int* st = d_status ? d_status : sd.status;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, dparams, S, K, d, &dv)) return frc;
  if (int rc = predict_run(h, dX, n, d, dy, dv, dXtest, m, sigma2, t.mean, t.var, d_beta, st)) return rc;
  launch_predict_summary(h->stream, t.mean, t.var, st, S, m, probs, n_probs, d_y_at, t.idx, t.count, d_out);
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
} CCGP_GUARD_END(h)

int ccgp_predict_summary(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                         const double* params, int S, const double* Xtest, int m, double sigma2,
                         const double* probs, int n_probs, const double* y_at, double* out,
                         double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || S < 1 || !X || !y || !params || !Xtest || !out)
    return fail(h, CCGP_EINVAL, "ccgp_predict_summary: bad argument");
  if (int rc = check_summary_args(h, m, probs, n_probs)) return rc;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  SummaryStage s;
  if (int rc = stage(h, [&](Layout& c) { s = summary_stage(c, n, d, P, S, m, n_probs); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.in.params, S, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(X, y, params, Xtest, y_at))) return prc;
  if (int rc = predict_run(h, s.in.X, n, d, s.in.y, dv, s.in.Xtest, m, sigma2, s.t.mean, s.t.var, s.beta, s.status)) return rc;
  launch_predict_summary(h->stream, s.t.mean, s.t.var, s.status, S, m, probs, n_probs, y_at ? s.y_at : nullptr, s.t.idx,
                         s.t.count, s.out);
  CCGP_LAUNCH_CHECK();
  return pull_status(h, s.results(out, out_beta), s.status, S, status);
} CCGP_GUARD_END(h)

// ---- the Combined GP's and the single GP's prediction over many training sets of one shape (ccgp.h) ---------------------------
// One call for the rows of C sets: every set's design, responses, test sites and rows go up in ONE span, the single-set
// launches (predict_run: whichever route the single-set call takes for the set's rows) run set after set on the resident
// inputs with no host copy between them, and the results come down in ONE span.  (predict_run itself may synchronise: it
// grows the workspace where the kept-factor scratch needs it -- once, the sets have one shape -- and forks and joins the
// second stream per set as the single-set call does.)  A set's rows are staged in their order as the nb x P table the
// single-set call stages, each piece with the alignment it has there, so the launches of set c are those of the single-set
// call on its rows: hence the bits.  The staging (call_stage.h: predict_sets_stage) holds every set's inputs and tables at
// once and is not cut over rows: the workspace limit governs predict_run's scratch, not this buffer.
enum class SetsOp { Predict, Krige, Summary };

// The one-launch route of the three calls (small_route_predict_sets == Reg, CCGP_OPT_PREDICT_FACTOR on, scratch to be had): the
// rows grouped by set go up with every set's design, responses and test sites in ONE span; per chunk of rows (the kept-factor
// scratch, capped as in kept_factor_ws_bytes) ONE factorisation launch, one correlation launch and one site launch serve the
// rows of all sets; a summary then runs its (site, set) grids on the whole tables; ONE span comes down.  *ran = false: the
// scratch could not be had and nothing was done -- the caller takes the grouped route.
static int predict_sets_one_launch(ccgp_handle* h, SetsOp op, const double* Xs, int n, int d, const double* ys,
                                   const double* sigma2, int C, int K, const double* params,
                                   const std::vector<std::vector<int>>& rows_of, int B, const double* sigma2_row, int var_form,
                                   const double* Xtests, int m, const double* probs, int n_probs, const double* ys_at,
                                   double* out_mean, double* out_var, double* out_summary, double* out_beta, double* out_q,
                                   int* status, bool* ran) {
  *ran = false;
  const size_t want = kept_factor_ws_bytes(h, true, n, d, K, B, m);
  if (!want || ensure(h, h->ws, kWorkspace, want) != CCGP_OK || h->ws.bytes < small_reg_sites_scratch(n, d, K, m)) return CCGP_OK;
  *ran = true;
  const int P = K + K * d;
  const bool summary = op == SetsOp::Summary, krige = op == SetsOp::Krige;
  const bool s2row = !krige || sigma2_row != nullptr;   // the Combined GP's sigma2 is its set's: one per row on the device
  const size_t nout = summary ? (size_t)m * (4 + n_probs) : 0;
  PredictSetsOneStage s;
  if (int rc = stage(h, [&](Layout& w) {
        s = predict_sets_one_stage(w, n, d, P, C, B, m, krige, s2row, summary, summary && ys_at, nout);
      }))
    return rc;
  // the grouped host images
  std::vector<int> order, hset(B), hoff(C), hnb(C);
  order.reserve(B);
  bool any_staged = false, any_streamed = false;
  for (int c = 0; c < C; ++c) {
    hoff[c] = (int)order.size();
    hnb[c] = (int)rows_of[c].size();
    if (hnb[c]) (hnb[c] <= kSummaryLdsDraws ? any_staged : any_streamed) = true;
    for (int b : rows_of[c]) { hset[order.size()] = c; order.push_back(b); }
  }
  std::vector<double> hp((size_t)B * P), hs2(s2row ? B : 0), hs2set(C, 1.0);
  for (int j = 0; j < P; ++j)
    for (int r = 0; r < B; ++r) hp[r + (size_t)j * B] = params[order[r] + (size_t)j * B];
  for (int r = 0; r < B && s2row; ++r) hs2[r] = krige ? sigma2_row[order[r]] : sigma2[hset[r]];
  if (!krige)
    for (int c = 0; c < C; ++c) hs2set[c] = sigma2[c];
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, B, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(Xs, ys, hs2set.data(), Xtests, hset.data(), hoff.data(), hnb.data(), hp.data(),
                                 s2row ? hs2.data() : nullptr, ys_at)))
    return prc;
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    (void)ensure_aux(h);
    const VarForm vf{s.s2row, krige ? var_form : VarForm{}.form, s.q};
    launch_small_reg_predict_sets(h->stream, s.Xs, n, d, s.ys, s.sigma2_set, s.set, dv, B, s.Xtests, m, s.mean, s.var, s.beta,
                                  s.status, h->ws.ptr, h->ws.bytes, h->aux_stream, h->aux_fork, h->aux_join, vf);
  }
  CCGP_LAUNCH_CHECK();
  if (summary) {
    launch_predict_summary_sets(h->stream, s.mean, s.var, s.status, B, m, C, s.off, s.nb, any_staged, any_streamed, probs,
                                n_probs, s.y_at, s.idx, s.count, s.out);
    CCGP_LAUNCH_CHECK();
  }
  std::vector<double> hmean(summary ? 0 : (size_t)B * m), hvar(summary ? 0 : (size_t)B * m), hbeta(B), hq(krige ? B : 0);
  std::vector<int> hst(B);
  if (int rc = pull(h, s.results(summary ? nullptr : hmean.data(), summary ? nullptr : hvar.data(), out_summary, hbeta.data(),
                                 krige ? hq.data() : nullptr, hst.data())))
    return rc;
  int failed = 0;
  for (int c = 0; c < C && summary; ++c)
    if (!hnb[c])   // no row: the S' = 0 rule of the single-set summary (the kernels leave the block alone)
      for (size_t e = 0; e < nout; ++e) out_summary[(size_t)c * nout + e] = std::nan("");
  for (int r = 0; r < B; ++r) {
    const int b = order[r];
    if (!summary)
      for (int t = 0; t < m; ++t) {
        out_mean[b + (size_t)t * B] = hmean[r + (size_t)t * B];
        out_var[b + (size_t)t * B] = hvar[r + (size_t)t * B];
      }
    if (out_beta) out_beta[b] = hbeta[r];
    if (out_q) out_q[b] = hq[r];
    if (status) status[b] = hst[r];
    failed += hst[r] != 0;
  }
  return failed;
}

static int predict_sets_call(ccgp_handle* h, SetsOp op, const double* Xs, int n, int d, const double* ys,
                             const double* sigma2, int C, int K, const double* params, const int* set, int B,
                             const double* sigma2_row, int var_form, const double* Xtests, int m, const double* probs,
                             int n_probs, const double* ys_at, double* out_mean, double* out_var, double* out_summary,
                             double* out_beta, double* out_q, int* status) {
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  const bool summary = op == SetsOp::Summary, krige = op == SetsOp::Krige;
  const size_t nout = summary ? (size_t)m * (4 + n_probs) : 0;
  std::vector<std::vector<int>> rows_of(C);
  for (int b = 0; b < B; ++b) rows_of[set[b]].push_back(b);
  if (h->fam.id == 0 && h->opt_predict_factor && small_route_predict_sets(true, n, d, K) == Route::Reg) {
    bool ran = false;
    const int rc = predict_sets_one_launch(h, op, Xs, n, d, ys, sigma2, C, K, params, rows_of, B, sigma2_row, var_form, Xtests, m,
                                           probs, n_probs, ys_at, out_mean, out_var, out_summary, out_beta, out_q, status, &ran);
    if (ran || rc < 0) return rc;
  }
  // the grouped route: set after set through the single-set launches
  std::vector<int> nb_of(C);
  for (int c = 0; c < C; ++c) nb_of[c] = (int)rows_of[c].size();
  std::vector<SetPieces> sp;
  if (int rc = stage(h, [&](Layout& w) {
        sp = predict_sets_stage(w, nb_of, n, d, P, m, krige, krige && sigma2_row, summary, summary && ys_at, nout);
      }))
    return rc;
  // the grouped host images: a set's rows as an nb x P column-major table, its per-row sigma2
  std::vector<double> hp((size_t)B * P), hs2(krige && sigma2_row ? B : 0);
  std::vector<Piece> up;
  for (int c = 0; c < C; ++c) {
    const SetPieces& s = sp[c];
    if (!s.nb) continue;
    double* rows = hp.data() + (size_t)s.off * P;
    for (int j = 0; j < P; ++j)
      for (int i = 0; i < s.nb; ++i) rows[i + (size_t)j * s.nb] = params[rows_of[c][i] + (size_t)j * B];
    for (int i = 0; i < s.nb && !hs2.empty(); ++i) hs2[s.off + i] = sigma2_row[rows_of[c][i]];
    up.push_back(piece(s.X, Xs + (size_t)c * n * d, (size_t)n * d));
    up.push_back(piece(s.y, ys + (size_t)c * n, n));
    up.push_back(piece(s.params, rows, (size_t)s.nb * P));
    up.push_back(piece(s.Xt, Xtests + (size_t)c * m * d, (size_t)m * d));
    if (s.s2row) up.push_back(piece(s.s2row, hs2.data() + s.off, (size_t)s.nb));
    if (s.y_at) up.push_back(piece(s.y_at, ys_at + (size_t)c * m, m));
  }
  if (int prc = push(h, up)) return prc;
  for (int c = 0; c < C; ++c) {
    const SetPieces& s = sp[c];
    if (!s.nb) continue;
    DrawView dv;
    if (int frc = draw_view(h, h->fam, s.params, s.nb, K, d, &dv)) return frc;
    const VarForm vf = krige ? VarForm{s.s2row, var_form, s.q} : VarForm{};
    if (int rc = predict_run(h, s.X, n, d, s.y, dv, s.Xt, m, krige ? 1.0 : sigma2[c], s.mean, s.var, s.beta, s.status, vf))
      return rc;
    if (summary) {
      launch_predict_summary(h->stream, s.mean, s.var, s.status, s.nb, m, probs, n_probs, s.y_at, s.idx, s.count, s.out);
      CCGP_LAUNCH_CHECK();
    }
  }
  // one span down, into grouped host images; then every row to its place among the B
  const bool tables = !summary;
  std::vector<double> hmean(tables ? (size_t)B * m : 0), hvar(tables ? (size_t)B * m : 0), hbeta(B), hq(krige ? B : 0);
  std::vector<int> hst(B);
  std::vector<Piece> down;
  for (int c = 0; c < C; ++c) {
    const SetPieces& s = sp[c];
    if (!s.nb) continue;
    const size_t nb = (size_t)s.nb;
    if (tables) {
      down.push_back(piece(s.mean, hmean.data() + (size_t)s.off * m, nb * m));
      down.push_back(piece(s.var, hvar.data() + (size_t)s.off * m, nb * m));
    } else {
      down.push_back(piece(s.out, out_summary + (size_t)c * nout, nout));
    }
    down.push_back(piece(s.beta, hbeta.data() + s.off, nb));
    if (krige) down.push_back(piece(s.q, hq.data() + s.off, nb));
    down.push_back(piece(s.status, hst.data() + s.off, nb));
  }
  if (int rc = pull(h, down)) return rc;
  int failed = 0;
  for (int c = 0; c < C; ++c) {
    const SetPieces& s = sp[c];
    if (!s.nb) {   // no row: the S' = 0 rule of the single-set summary
      for (size_t e = 0; e < nout; ++e) out_summary[(size_t)c * nout + e] = std::nan("");
      continue;
    }
    for (int i = 0; i < s.nb; ++i) {
      const int b = rows_of[c][i];
      if (tables)
        for (int t = 0; t < m; ++t) {
          out_mean[b + (size_t)t * B] = hmean[(size_t)s.off * m + i + (size_t)t * s.nb];
          out_var[b + (size_t)t * B] = hvar[(size_t)s.off * m + i + (size_t)t * s.nb];
        }
      if (out_beta) out_beta[b] = hbeta[s.off + i];
      if (out_q) out_q[b] = hq[s.off + i];
      if (status) status[b] = hst[s.off + i];
      failed += hst[s.off + i] != 0;
    }
  }
  return failed;
}

int ccgp_predict_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                            int K, const double* params, const int* set, int B, const double* Xtests, int m,
                            double* out_mean, double* out_var, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || m < 1 || !params || !Xtests || !out_mean || !out_var ||
      !sets_args_ok(Xs, ys, sigma2, true, C, set, B, 1))
    return fail(h, CCGP_EINVAL, "ccgp_predict_batch_sets: bad argument");
  return predict_sets_call(h, SetsOp::Predict, Xs, n, d, ys, sigma2, C, K, params, set, B, nullptr, 0,
                           Xtests, m, nullptr, 0, nullptr, out_mean, out_var, nullptr, out_beta, nullptr, status);
} CCGP_GUARD_END(h)

int ccgp_krige_predict_batch_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, int C, int K,
                                  const double* params, const int* set, int B, const double* sigma2_row, int var_form,
                                  const double* Xtests, int m, double* out_mean, double* out_var, double* out_beta,
                                  double* out_q, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || m < 1 || !params || !Xtests || !out_mean || !out_var ||
      !sets_args_ok(Xs, ys, nullptr, false, C, set, B, 1))
    return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch_sets: bad argument");
  // what ccgp_krige_predict_batch refuses
  if (var_form != CCGP_VAR_ORDINARY && var_form != CCGP_VAR_PLUGIN && var_form != CCGP_VAR_UNBIASED)
    return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch_sets: unknown var_form");
  const bool own_s2 = var_form != CCGP_VAR_UNBIASED;
  if (!own_s2 && n < 2) return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch_sets: CCGP_VAR_UNBIASED divides by n - 1");
  if (own_s2) {
    if (!sigma2_row) return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch_sets: this var_form needs sigma2");
    for (int b = 0; b < B; ++b)
      if (!(std::isfinite(sigma2_row[b]) && sigma2_row[b] >= 0.0))
        return fail(h, CCGP_EINVAL, "ccgp_krige_predict_batch_sets: every sigma2 must be finite and >= 0");
  }
  return predict_sets_call(h, SetsOp::Krige, Xs, n, d, ys, nullptr, C, K, params, set, B,
                           own_s2 ? sigma2_row : nullptr, var_form, Xtests, m, nullptr, 0, nullptr, out_mean, out_var, nullptr,
                           out_beta, out_q, status);
} CCGP_GUARD_END(h)

int ccgp_predict_summary_sets(ccgp_handle* h, const double* Xs, int n, int d, const double* ys, const double* sigma2, int C,
                              int K, const double* params, const int* set, int B, const double* Xtests, int m,
                              const double* probs, int n_probs, const double* ys_at, double* out, double* out_beta,
                              int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || !params || !Xtests || !out || !sets_args_ok(Xs, ys, sigma2, true, C, set, B, 1))
    return fail(h, CCGP_EINVAL, "ccgp_predict_summary_sets: bad argument");
  if (int rc = check_summary_args(h, m, probs, n_probs)) return rc;
  return predict_sets_call(h, SetsOp::Summary, Xs, n, d, ys, sigma2, C, K, params, set, B, nullptr, 0,
                           Xtests, m, probs, n_probs, ys_at, nullptr, nullptr, out, out_beta, nullptr, status);
} CCGP_GUARD_END(h)

// ---- leave-one-out cross-validation of the Combined GP: the closed form from ONE factorisation per draw ---------------
// the tables of the B draws of dv on resident inputs; arguments are checked by the callers.  vf.q is never nullptr.  The
// route is asked once (small_route_loo): the fourth inverse instance of small_reg.hip, timed under CCGP_T_FUSED, or identity
// rows on the blocked sweep with loo_kernel behind it, timed under CCGP_T_SOLVE.
static int loo_run(ccgp_handle* h, const double* dX, int n, int d, const double* dy, const DrawView& dv, double sigma2,
                   VarForm vf, double* d_mean, double* d_var, double* d_beta, int* d_status) {
  const int K = dv.K, B = dv.ldp;
  if (small_route_loo(gauss_or_fused_loo(h, dv.fam, n, d, K), n, d, K) == Route::Blocked) {
    const int npad = round_up(n, kTile);
    SweepOut sc{};
    BlockedJob job{};
    job.kind = kJobLoo; job.S = B; job.mean = d_mean; job.var = d_var; job.vf = vf;
    return run_sweep(h, dX, n, d, dy, dv, B, npad / kTile, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, sc, &job, 0,
                     [&](Layout& t, int) { sc = predict_tail(t, B, d_beta, d_status); });
  }
  {
    ScopedTimer t(h, CCGP_T_FUSED);
    launch_small_reg_loo(h->stream, dX, n, d, dy, dv, B, sigma2, vf, d_mean, d_var, d_beta, d_status);
  }
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}

int ccgp_loo_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K, const double* params, int B,
                   const double* sigma2, int var_form, double* out_mean, double* out_var, double* out_beta, double* out_q,
                   int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || B < 0 || !X || !y || !params || !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_loo_batch: bad argument");
  if (var_form != CCGP_VAR_ORDINARY && var_form != CCGP_VAR_PLUGIN && var_form != CCGP_VAR_UNBIASED)
    return fail(h, CCGP_EINVAL, "ccgp_loo_batch: unknown var_form");
  const bool own_s2 = var_form != CCGP_VAR_UNBIASED;
  if (n < 2) return fail(h, CCGP_EINVAL, "ccgp_loo_batch: a fold needs at least one other point (n >= 2)");
  if (!own_s2 && n < 3) return fail(h, CCGP_EINVAL, "ccgp_loo_batch: CCGP_VAR_UNBIASED divides by n - 2");
  if (own_s2) {
    if (!sigma2) return fail(h, CCGP_EINVAL, "ccgp_loo_batch: this var_form needs sigma2");
    for (int b = 0; b < B; ++b)
      if (!(std::isfinite(sigma2[b]) && sigma2[b] >= 0.0))
        return fail(h, CCGP_EINVAL, "ccgp_loo_batch: every sigma2 must be finite and >= 0");
  }
  if (B == 0) return CCGP_OK;
  CCGP_HIP(hipSetDevice(h->device));
  LooStage s;
  if (int rc = stage(h, [&](Layout& c) { s = loo_stage(c, n, d, K + K * d, B, own_s2); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, B, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(X, y, params, own_s2 ? sigma2 : nullptr))) return prc;
  if (int rc = loo_run(h, s.X, n, d, s.y, dv, 1.0, VarForm{s.sigma2, var_form, s.q}, s.mean, s.var, s.beta, s.status)) return rc;
  return pull_status(h, s.results(out_mean, out_var, out_beta, out_q), s.status, B, status);
} CCGP_GUARD_END(h)

int ccgp_loo_summary(ccgp_handle* h, const double* X, int n, int d, const double* y, int K, const double* params, int S,
                     double sigma2, const double* probs, int n_probs, double* out, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || n < 2 || S < 1 || !X || !y || !params || !out || !(std::isfinite(sigma2) && sigma2 >= 0.0))
    return fail(h, CCGP_EINVAL, "ccgp_loo_summary: bad argument");
  if (int rc = check_summary_args(h, n, probs, n_probs)) return rc;
  CCGP_HIP(hipSetDevice(h->device));
  LooSummaryStage s;
  if (int rc = stage(h, [&](Layout& c) { s = loo_summary_stage(c, n, d, K + K * d, S, n_probs); })) return rc;
  DrawView dv;
  if (int frc = draw_view(h, h->fam, s.params, S, K, d, &dv)) return frc;
  if (int prc = push(h, s.inputs(X, y, params))) return prc;
  if (int rc = loo_run(h, s.X, n, d, s.y, dv, sigma2, VarForm{nullptr, CCGP_VAR_ORDINARY, s.q}, s.t.mean, s.t.var, s.beta,
                       s.status))
    return rc;
  // the sites are the training points and y_at the resident y: column 3 is the PIT value F(y_i)
  launch_predict_summary(h->stream, s.t.mean, s.t.var, s.status, S, n, probs, n_probs, s.y, s.t.idx, s.t.count, s.out);
  CCGP_LAUNCH_CHECK();
  return pull_status(h, s.results(out, out_beta), s.status, S, status);
} CCGP_GUARD_END(h)

// ---- 8(f)-2: device-resident factor set --------------------------------------------------------------
struct ccgp_factorset {
  int device = 0;
  int n = 0, d = 0, K = 0, S = 0, npad = 0;
  double sigma2 = 0.0;
  ccgp::KernelFamily fam;
  bool fused = false;      // n <= 128: nothing but the draws is kept (see ccgp_factor_batch)
  void* mem = nullptr;
  size_t bytes = 0;
  double* X = nullptr;     // device copies
  double* y = nullptr;
  double* params = nullptr;
  double* ll = nullptr;
  double* beta = nullptr;
  int* status = nullptr;
  ccgp::BlockedWs w{};
};

// owner of a factor set and of its device memory
struct FactorsetFree {
  ccgp_handle* h;   // the handle whose last scheduled sweep may have left its time account in the set; may be nullptr
  void operator()(ccgp_factorset* fs) const {
    if (h) forget_sched_profile(h, fs->mem, fs->bytes);
    if (fs->mem) (void)hipFree(fs->mem);
    delete fs;
  }
};

int ccgp_factor_batch(ccgp_handle* h, const double* X, int n, int d, const double* y, int K,
                      const double* params, int S, double sigma2, ccgp_factorset** out,
                      double* out_loglik, double* out_beta, int* status) try {
  if (!h) return CCGP_EINVAL;
  if (bad_shape(n, d, K) || S < 1 || !X || !y || !params || !out)
    return fail(h, CCGP_EINVAL, "ccgp_factor_batch: bad argument");
  *out = nullptr;
  DrawView dv;   // its params follow once the set has its memory
  if (int frc = draw_view(h, h->fam, nullptr, S, K, d, &dv)) return frc;
  CCGP_HIP(hipSetDevice(h->device));
  const int P = K + K * d;
  const bool fused = small_route(Op::Predict, h->fam.id == 0, n, d, K) == Route::Reg;
  const int npad = round_up(n, kTile);
  if (!fused && S > 65535)   // the draw index is a grid y / z dimension in cov_kernel, rhs_rows_kernel, ...
    return fail(h, CCGP_EINVAL, "ccgp_factor_batch: at most 65535 factors per set on the blocked path (n > 128)");
  std::unique_ptr<ccgp_factorset, FactorsetFree> fs(new ccgp_factorset(), FactorsetFree{h});
  char* factors = nullptr;
  auto lay = [&](Layout& c) {
    fs->X = c.take<double>((size_t)n * d);
    fs->y = c.take<double>(n);
    fs->params = c.take<double>((size_t)S * P);
    fs->ll = c.take<double>(S);
    fs->beta = c.take<double>(S);
    fs->status = c.take<int>(S);
    if (!fused) factors = c.take<char>(blocked_ws_bytes(npad, S, 0));
  };
  const size_t bytes = layout_bytes(lay);
  if (hipMalloc(&fs->mem, bytes) != hipSuccess) {
    fs->mem = nullptr;
    return fail(h, CCGP_ENOMEM, "ccgp_factor_batch: " + std::to_string(bytes) + " B for " + std::to_string(S) +
                                    " factors do not fit on the device");
  }
  if (h->debug_fill >= 0)
    if (int rc = debug_fill(h, fs->mem, bytes, false, h->debug_fill)) return rc;
  fs->bytes = bytes; fs->device = h->device; fs->n = n; fs->d = d; fs->K = K; fs->S = S; fs->npad = npad;
  fs->sigma2 = sigma2; fs->fam = h->fam; fs->fused = fused;
  Layout c(fs->mem);
  lay(c);
  dv.params = fs->params;
  if (int prc = push(h, {piece(fs->X, X, (size_t)n * d), piece(fs->y, y, n), piece(fs->params, params, (size_t)S * P)}))
    return prc;
  CCGP_HIP(hipMemsetAsync(fs->status, 0, sizeof(int) * (size_t)S, h->stream));
  if (fused) {
    // n <= 128: the factor of a draw lives and dies in registers / LDS inside the fused evaluator (10 us);
    // storing it would cost more HBM traffic than regenerating it.  The set keeps the draws; likelihood
    // and beta are evaluated once here, prediction re-runs the fused predictor on the resident inputs.
    if (int rc = loglik_run(h, fs->X, n, d, fs->y, dv, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, fs->ll, fs->beta, fs->status))
      return rc;
  } else {
    fs->w = blocked_carve(factors, npad, S, 0);
    blocked_loglik(h, fs->X, n, d, fs->y, dv, 0, S, npad, sigma2, CCGP_MEAN_PROFILE_BETA, 0.0, fs->w, fs->ll,
                   fs->beta, fs->status);
    CCGP_LAUNCH_CHECK();
  }
  const int failed = pull_status(h, {piece(fs->ll, out_loglik, S), piece(fs->beta, out_beta, S)}, fs->status, S, status);
  if (failed >= 0) *out = fs.release();
  return failed;
} CCGP_GUARD_END(h)

// the S x m tables of a factor set at the m resident test sites dXt; arguments are checked by the callers
static int factorset_predict_run(ccgp_handle* h, const ccgp_factorset* fs, const double* dXt, int m, double* dmean,
                                 double* dvar) {
  const int n = fs->n, d = fs->d, S = fs->S;
  DrawView dv;   // the set's kernel family, whatever the handle has been set to since
  if (int frc = draw_view(h, fs->fam, fs->params, S, fs->K, d, &dv)) return frc;
  if (fs->fused) return predict_run(h, fs->X, n, d, fs->y, dv, dXt, m, fs->sigma2, dmean, dvar, nullptr, nullptr);
  const int ne = (m + kTile - 1) / kTile, lde = ne * kTile;
  const size_t e_stride = (size_t)lde * fs->npad;
  // the m cross-correlation rows of every draw need lde x npad doubles of scratch: chunks of draws
  int sc = 0;
  if (int rc = plan_chunk(h, sizeof(double) * e_stride, S, kFactorsetMargin,
                          [&](int ns) { return sizeof(double) * e_stride * (size_t)ns; }, &sc))
    return rc;
  double* E = static_cast<double*>(h->ws.ptr);
  for (int s0 = 0; s0 < S; s0 += sc) {
    const int ns = std::min(sc, S - s0);
    CCGP_HIP(hipMemsetAsync(E, 0, sizeof(double) * e_stride * ns, h->stream));
    {
      ScopedTimer t(h, CCGP_T_COV);   // rows t = r(x_t)' (Mixed.corr.vec, HX:425-431)
      launch_cov_cross_batched(h->stream, dXt, m, fs->X, n, d, dv, s0, ns, E, e_stride, lde);
    }
    blocked_predict_from_factors(h, fs->w, n, fs->npad, S, s0, ns, E, e_stride, lde, m, fs->status, fs->sigma2, dmean, dvar);
  }
  CCGP_LAUNCH_CHECK();
  return CCGP_OK;
}

int ccgp_predict_from_factorset(ccgp_handle* h, const ccgp_factorset* fs, const double* Xtest, int m,
                                double* out_mean, double* out_var) try {
  if (!h) return CCGP_EINVAL;
  if (!fs || !Xtest || m < 1 || !out_mean || !out_var)
    return fail(h, CCGP_EINVAL, "ccgp_predict_from_factorset: bad argument");
  if (fs->device != h->device)
    return fail(h, CCGP_EINVAL, "ccgp_predict_from_factorset: the factor set lives on another device");
  CCGP_HIP(hipSetDevice(h->device));
  const int d = fs->d, S = fs->S;
  double *dXt, *dmean, *dvar;
  if (int rc = stage(h, [&](Layout& c) {
        dXt = c.take<double>((size_t)m * d);
        dmean = c.take<double>((size_t)S * m);
        dvar = c.take<double>((size_t)S * m);
      }))
    return rc;
  if (int prc = push(h, {piece(dXt, Xtest, (size_t)m * d)})) return prc;
  if (int rc = factorset_predict_run(h, fs, dXt, m, dmean, dvar)) return rc;
  return pull(h, {piece(dmean, out_mean, (size_t)S * m), piece(dvar, out_var, (size_t)S * m)});
} CCGP_GUARD_END(h)

int ccgp_summary_from_factorset(ccgp_handle* h, const ccgp_factorset* fs, const double* Xtest, int m,
                                const double* probs, int n_probs, const double* y_at, double* out) try {
  if (!h) return CCGP_EINVAL;
  if (!fs || !Xtest || !out) return fail(h, CCGP_EINVAL, "ccgp_summary_from_factorset: bad argument");
  if (int rc = check_summary_args(h, m, probs, n_probs)) return rc;
  if (fs->device != h->device)
    return fail(h, CCGP_EINVAL, "ccgp_summary_from_factorset: the factor set lives on another device");
  CCGP_HIP(hipSetDevice(h->device));
  const int d = fs->d, S = fs->S;
  double *dXt, *dy_at, *dout;
  SummaryTables t;
  if (int rc = stage(h, [&](Layout& c) {
        dXt = c.take<double>((size_t)m * d);
        dy_at = c.take<double>(m);
        t = summary_tables(c, S, m);
        dout = c.take<double>((size_t)m * (4 + n_probs));
      }))
    return rc;
  if (int prc = push(h, {piece(dXt, Xtest, (size_t)m * d), piece(dy_at, y_at, m)})) return prc;
  if (int rc = factorset_predict_run(h, fs, dXt, m, t.mean, t.var)) return rc;
  launch_predict_summary(h->stream, t.mean, t.var, fs->status, S, m, probs, n_probs, y_at ? dy_at : nullptr, t.idx,
                         t.count, dout);
  CCGP_LAUNCH_CHECK();
  int valid = 0;   // t.count closes the tables, dout follows it: one span down
  if (int rc = pull(h, {piece(t.count, &valid, 1), piece(dout, out, (size_t)m * (4 + n_probs))})) return rc;
  return S - valid;
} CCGP_GUARD_END(h)

size_t ccgp_factorset_bytes(const ccgp_factorset* fs) { return fs ? fs->bytes : 0; }

int ccgp_factorset_free(ccgp_handle* h, ccgp_factorset* fs) try {
  if (!fs) return CCGP_OK;
  if (h) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
  }
  FactorsetFree{h}(fs);
  return CCGP_OK;
} CCGP_GUARD_END(h)

}  // extern "C"
