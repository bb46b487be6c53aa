// What the host-pointer entry points of capi.hip declare before they touch the device: the pieces a copy moves (Piece,
// span_of) and the staging layouts that ccgp_reserve or more than one entry point needs.  Each layout is ONE declaration
// over a Layout (stage_layout.h) and says itself which of its pieces go up (inputs) and which come back (results), so a
// call's buffer size, its pointers and its copies cannot disagree.  One-off layouts stay as lambdas at their call site.
// No HIP include: the CPU suite runs these declarations with the host compiler (tests/host_stage).
#pragma once

#include <cstddef>
#include <initializer_list>
#include <vector>

#include "stage_layout.h"

namespace ccgp {

struct Piece {
  void* dev;
  void* host;      // source for push, destination for pull; nullptr: skip
  size_t bytes;
};
template <class T>
Piece piece(T* dev, const T* host, size_t count) {
  return Piece{dev, const_cast<T*>(host), sizeof(T) * count};
}
struct Pieces {   // a braced list at the call site, or a vector
  const Piece *b, *e;
  Pieces(std::initializer_list<Piece> l) { b = l.begin(); e = l.end(); }   // both live to the end of the call's expression
  Pieces(const std::vector<Piece>& v) { b = v.data(); e = v.data() + v.size(); }
  const Piece* begin() const { return b; }
  const Piece* end() const { return e; }
};

// the device range [lo, lo + bytes) that covers the pieces a copy moves; lo == nullptr: none moves
struct Span {
  char* lo = nullptr;
  size_t bytes = 0;
};
inline Span span_of(Pieces ps) {
  char *lo = nullptr, *hi = nullptr;
  for (const Piece& p : ps) {
    if (!p.host || !p.bytes) continue;
    char* d = static_cast<char*>(p.dev);
    if (!lo || d < lo) lo = d;
    if (!hi || d + p.bytes > hi) hi = d + p.bytes;
  }
  return Span{lo, (size_t)(hi - lo)};
}

// ---- ccgp_loglik_batch: inputs X | y | params and results loglik | beta | status, each ONE piece, so that each side
// crosses PCIe as one span
struct LoglikStage {
  double *X = nullptr, *y = nullptr, *params = nullptr, *loglik = nullptr, *beta = nullptr;
  int* status = nullptr;
  size_t payload = 0;   // bytes of the two pieces
};
inline LoglikStage loglik_stage(Layout& c, int n, int d, int P, int B) {
  const size_t in_d = (size_t)n * d + n + (size_t)B * P, out_d = 2 * (size_t)B + ((size_t)B + 1) / 2;
  double* in = c.take<double>(in_d);
  double* out = c.take<double>(out_d);
  LoglikStage s;
  s.payload = sizeof(double) * (in_d + out_d);
  if (!in) return s;   // planning pass
  s.X = in;
  s.y = in + (size_t)n * d;
  s.params = s.y + n;
  s.loglik = out;
  s.beta = out + B;
  s.status = reinterpret_cast<int*>(out + 2 * (size_t)B);
  return s;
}

// ---- ccgp_loglik_grad_batch and ccgp_profile_batch: X | y | params | grad? | loglik | s2hat? | beta | status | gpart?
// the device outputs of a value-and-gradient evaluation (grad_run).  s2hat set: the profiled mode; grad == nullptr: value
// only, legal in the profiled mode alone; gpart: the partial sums of launch_small_grad, read on the in-LDS route only
struct GradOut {
  double *loglik, *beta;
  int* status;
  double *grad, *s2hat, *gpart;
};
struct GradStage {
  double *X, *y, *params;
  GradOut o;
  size_t nX, ny, nparams, B;
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams) const {
    return {piece(X, hX, nX), piece(y, hy, ny), piece(params, hparams, nparams)};
  }
  // the status words follow them (pull_status)
  std::vector<Piece> results(double* grad, double* loglik, double* s2hat, double* beta) const {
    return {piece(o.grad, grad, o.grad ? nparams : 0), piece(o.loglik, loglik, B), piece(o.s2hat, s2hat, o.s2hat ? B : 0),
            piece(o.beta, beta, B)};
  }
};
inline GradStage grad_stage(Layout& c, int n, int d, int P, int B, bool grad, bool s2hat, size_t gpart_doubles) {
  GradStage s;
  s.nX = (size_t)n * d; s.ny = n; s.nparams = (size_t)B * P; s.B = B;
  s.X = c.take<double>(s.nX);
  s.y = c.take<double>(s.ny);
  s.params = c.take<double>(s.nparams);
  s.o.grad = grad ? c.take<double>(s.nparams) : nullptr;
  s.o.loglik = c.take<double>(B);
  s.o.s2hat = s2hat ? c.take<double>(B) : nullptr;
  s.o.beta = c.take<double>(B);
  s.o.status = c.take<int>(B);
  s.o.gpart = gpart_doubles ? c.take<double>(gpart_doubles) : nullptr;
  return s;
}

// ---- prediction: the four inputs every host-pointer prediction call stages and pushes
struct PredictIn {
  double *X, *y, *params, *Xtest;
  size_t nX, ny, nparams, nXtest;
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams, const double* hXtest) const {
    return {piece(X, hX, nX), piece(y, hy, ny), piece(params, hparams, nparams), piece(Xtest, hXtest, nXtest)};
  }
};
inline PredictIn predict_in(Layout& c, int n, int d, int P, int S, int m) {
  PredictIn s;
  s.nX = (size_t)n * d; s.ny = n; s.nparams = (size_t)S * P; s.nXtest = (size_t)m * d;
  s.X = c.take<double>(s.nX);
  s.y = c.take<double>(s.ny);
  s.params = c.take<double>(s.nparams);
  s.Xtest = c.take<double>(s.nXtest);
  return s;
}

// ccgp_predict_batch, and with the tail ccgp_krige_predict_batch: in | mean | var | beta | status | (sigma2 | q)?
struct PredictStage {
  PredictIn in;
  double *mean, *var, *beta;
  int* status;
  double *sigma2, *q;   // the per-row tail; nullptr without it
  size_t S, m;
  // sigma2: the per-row values that go up with the inputs (nullptr: none, or no tail)
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams, const double* hXtest,
                            const double* hsigma2) const {
    std::vector<Piece> ps = in.inputs(hX, hy, hparams, hXtest);
    ps.push_back(piece(sigma2, hsigma2, sigma2 ? S : 0));
    return ps;
  }
  // the status words follow beta (pull_status)
  std::vector<Piece> results(double* hmean, double* hvar, double* hbeta, double* hq) const {
    return {piece(mean, hmean, S * m), piece(var, hvar, S * m), piece(beta, hbeta, S), piece(q, hq, q ? S : 0)};
  }
};
inline PredictStage predict_stage(Layout& c, int n, int d, int P, int S, int m, bool tail = false) {
  PredictStage s;
  s.S = S; s.m = m;
  s.in = predict_in(c, n, d, P, S, m);
  s.mean = c.take<double>(s.S * s.m);
  s.var = c.take<double>(s.S * s.m);
  s.beta = c.take<double>(S);
  s.status = c.take<int>(S);
  s.sigma2 = tail ? c.take<double>(S) : nullptr;
  s.q = tail ? c.take<double>(S) : nullptr;
  return s;
}

// ---- the prediction summaries (summary.hip).  The S x m tables never leave the device: they lie BETWEEN the inputs (one
// span up) and the results (one span down), next to the scratch of the summary kernel.
struct SummaryTables {
  double *mean, *var;
  int *idx, *count;
};
inline SummaryTables summary_tables(Layout& c, int S, int m) {
  SummaryTables t;
  t.mean = c.take<double>((size_t)S * m);
  t.var = c.take<double>((size_t)S * m);
  t.idx = c.take<int>(S);
  t.count = c.take<int>(1);
  return t;
}
// ccgp_predict_summary: in | y_at | tables | out | beta | status
struct SummaryStage {
  PredictIn in;
  double* y_at;
  SummaryTables t;
  double *out, *beta;
  int* status;
  size_t S, m, nout;
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams, const double* hXtest,
                            const double* hy_at) const {
    std::vector<Piece> ps = in.inputs(hX, hy, hparams, hXtest);
    ps.push_back(piece(y_at, hy_at, m));
    return ps;
  }
  std::vector<Piece> results(double* hout, double* hbeta) const { return {piece(out, hout, nout), piece(beta, hbeta, S)}; }
};
inline SummaryStage summary_stage(Layout& c, int n, int d, int P, int S, int m, int n_probs) {
  SummaryStage s;
  s.S = S; s.m = m; s.nout = (size_t)m * (4 + n_probs);
  s.in = predict_in(c, n, d, P, S, m);
  s.y_at = c.take<double>(m);
  s.t = summary_tables(c, S, m);
  s.out = c.take<double>(s.nout);
  s.beta = c.take<double>(S);
  s.status = c.take<int>(S);
  return s;
}
// ccgp_predict_summary_dev: the tables and, where the caller keeps no status words, room for them
struct SummaryDevStage {
  SummaryTables t;
  int* status;
};
inline SummaryDevStage summary_dev_stage(Layout& c, int S, int m, bool own_status) {
  SummaryDevStage s;
  s.t = summary_tables(c, S, m);
  s.status = own_status ? c.take<int>(S) : nullptr;
  return s;
}

// ---- leave-one-out (ccgp_loo_batch, ccgp_loo_summary): the training points are the sites, so no test set goes up.
// ccgp_loo_batch: X | y | params | sigma2? | mean | var | beta | q | status.  Q is always staged: CCGP_VAR_UNBIASED reads it
// on the device whether or not the caller wants it back.
struct LooStage {
  double *X, *y, *params, *sigma2;
  double *mean, *var, *beta, *q;
  int* status;
  size_t nX, n, nparams, B;
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams, const double* hsigma2) const {
    return {piece(X, hX, nX), piece(y, hy, n), piece(params, hparams, nparams), piece(sigma2, hsigma2, sigma2 ? B : 0)};
  }
  // the status words follow q (pull_status)
  std::vector<Piece> results(double* hmean, double* hvar, double* hbeta, double* hq) const {
    return {piece(mean, hmean, B * n), piece(var, hvar, B * n), piece(beta, hbeta, B), piece(q, hq, B)};
  }
};
inline LooStage loo_stage(Layout& c, int n, int d, int P, int B, bool own_sigma2) {
  LooStage s;
  s.nX = (size_t)n * d; s.n = n; s.nparams = (size_t)B * P; s.B = B;
  s.X = c.take<double>(s.nX);
  s.y = c.take<double>(s.n);
  s.params = c.take<double>(s.nparams);
  s.sigma2 = own_sigma2 ? c.take<double>(B) : nullptr;
  s.mean = c.take<double>(s.B * s.n);
  s.var = c.take<double>(s.B * s.n);
  s.beta = c.take<double>(B);
  s.q = c.take<double>(B);
  s.status = c.take<int>(B);
  return s;
}
// ccgp_loo_summary: X | y | params | tables | q | out | beta | status -- the tables stay on the device, as in SummaryStage
struct LooSummaryStage {
  double *X, *y, *params;
  SummaryTables t;
  double *q, *out, *beta;
  int* status;
  size_t nX, n, nparams, S, nout;
  std::vector<Piece> inputs(const double* hX, const double* hy, const double* hparams) const {
    return {piece(X, hX, nX), piece(y, hy, n), piece(params, hparams, nparams)};
  }
  std::vector<Piece> results(double* hout, double* hbeta) const { return {piece(out, hout, nout), piece(beta, hbeta, S)}; }
};
inline LooSummaryStage loo_summary_stage(Layout& c, int n, int d, int P, int S, int n_probs) {
  LooSummaryStage s;
  s.nX = (size_t)n * d; s.n = n; s.nparams = (size_t)S * P; s.S = S; s.nout = (size_t)n * (4 + n_probs);
  s.X = c.take<double>(s.nX);
  s.y = c.take<double>(s.n);
  s.params = c.take<double>(s.nparams);
  s.t = summary_tables(c, S, n);
  s.q = c.take<double>(S);
  s.out = c.take<double>(s.nout);
  s.beta = c.take<double>(S);
  s.status = c.take<int>(S);
  return s;
}

// ---- the sets form of the likelihood (ccgp_loglik_batch_sets): C training sets of one shape go up with the B parameter rows
// and the set every row belongs to: Xs | ys | sigma2 | params | set | loglik | beta | status
struct SetsStage {
  double *Xs, *ys, *sigma2, *params;
  int* set;
  double *loglik, *beta;
  int* status;
  size_t nXs, nys, C, nparams, B;
  std::vector<Piece> inputs(const double* hXs, const double* hys, const double* hsigma2, const double* hparams,
                            const int* hset) const {
    return {piece(Xs, hXs, nXs), piece(ys, hys, nys), piece(sigma2, hsigma2, C), piece(params, hparams, nparams),
            piece(set, hset, B)};
  }
  // the status words follow beta (pull_status)
  std::vector<Piece> results(double* hloglik, double* hbeta) const { return {piece(loglik, hloglik, B), piece(beta, hbeta, B)}; }
};
inline SetsStage sets_stage(Layout& c, int n, int d, int P, int C, int B) {
  SetsStage s;
  s.nXs = (size_t)C * n * d; s.nys = (size_t)C * n; s.C = C; s.nparams = (size_t)B * P; s.B = B;
  s.Xs = c.take<double>(s.nXs);
  s.ys = c.take<double>(s.nys);
  s.sigma2 = c.take<double>(s.C);
  s.params = c.take<double>(s.nparams);
  s.set = c.take<int>(s.B);
  s.loglik = c.take<double>(s.B);
  s.beta = c.take<double>(s.B);
  s.status = c.take<int>(s.B);
  return s;
}

// ---- the chunked calls of the comparator fits (ccgp_profile_batch_sets with a gradient; ccgp_cgp_state_batch_sets and, as
// its C = 1 case that names no set, ccgp_cgp_state_batch).  A call is cut into chunks of nb rows (plan_chunk): the C training
// sets lie in front and go up ONCE, with the first chunk; behind them a chunk's rows, its set indices and its results, the
// inputs back to back so that they go up as one span.  `first`: this chunk is the call's first.
//   ccgp_profile_batch_sets: Xs | ys | set | params | grad | loglik | s2hat | beta | status
struct ProfileSetsStage {
  double *Xs, *ys;
  int* set;
  double *params, *grad, *loglik, *s2hat, *beta;
  int* status;
  size_t nXs, nys, P;
  std::vector<Piece> inputs(bool first, const double* hXs, const double* hys, const int* hset, const double* hparams,
                            int nb) const {
    return {piece(Xs, first ? hXs : nullptr, nXs), piece(ys, first ? hys : nullptr, nys), piece(set, hset, (size_t)nb),
            piece(params, hparams, (size_t)nb * P)};
  }
  // the status words follow beta (pull_status)
  std::vector<Piece> results(double* hgrad, double* hloglik, double* hs2hat, double* hbeta, int nb) const {
    return {piece(grad, hgrad, (size_t)nb * P), piece(loglik, hloglik, (size_t)nb), piece(s2hat, hs2hat, (size_t)nb),
            piece(beta, hbeta, (size_t)nb)};
  }
};
inline ProfileSetsStage profile_sets_stage(Layout& c, int n, int d, int P, int C, int nb) {
  ProfileSetsStage s;
  s.nXs = (size_t)C * n * d; s.nys = (size_t)C * n; s.P = P;
  s.Xs = c.take<double>(s.nXs);
  s.ys = c.take<double>(s.nys);
  s.set = c.take<int>(nb);
  s.params = c.take<double>((size_t)nb * P);
  s.grad = c.take<double>((size_t)nb * P);
  s.loglik = c.take<double>(nb);
  s.s2hat = c.take<double>(nb);
  s.beta = c.take<double>(nb);
  s.status = c.take<int>(nb);
  return s;
}
inline size_t profile_sets_row_bytes(int P) { return sizeof(double) * (2 * (size_t)P + 3) + 2 * sizeof(int); }
//   ccgp_cgp_state_batch[_sets]: Xs | ys | set | skip | params | val | beta | tau2 | loo | status
struct CgpSetsStage {
  double *Xs, *ys;
  int *set, *skip;
  double *params, *val, *beta, *tau2, *loo;
  int* status;
  size_t nXs, nys, P;
  std::vector<Piece> inputs(bool first, const double* hXs, const double* hys, const int* hset, const int* hskip,
                            const double* hparams, int nb) const {
    return {piece(Xs, first ? hXs : nullptr, nXs), piece(ys, first ? hys : nullptr, nys), piece(set, hset, (size_t)nb),
            piece(skip, hskip, (size_t)nb), piece(params, hparams, (size_t)nb * P)};
  }
  // the status words follow loo (pull_status)
  std::vector<Piece> results(double* hval, double* hbeta, double* htau2, double* hloo, int nb) const {
    return {piece(val, hval, (size_t)nb), piece(beta, hbeta, (size_t)nb), piece(tau2, htau2, (size_t)nb),
            piece(loo, hloo, (size_t)nb)};
  }
};
inline CgpSetsStage cgp_sets_stage(Layout& c, int n, int d, int C, int nb) {
  CgpSetsStage s;
  s.nXs = (size_t)C * n * d; s.nys = (size_t)C * n; s.P = 2 * (size_t)d + 2;
  s.Xs = c.take<double>(s.nXs);
  s.ys = c.take<double>(s.nys);
  s.set = c.take<int>(nb);
  s.skip = c.take<int>(nb);
  s.params = c.take<double>((size_t)nb * s.P);
  s.val = c.take<double>(nb);
  s.beta = c.take<double>(nb);
  s.tau2 = c.take<double>(nb);
  s.loo = c.take<double>(nb);
  s.status = c.take<int>(nb);
  return s;
}
inline size_t cgp_sets_row_bytes(int d) { return sizeof(double) * (2 * (size_t)d + 2 + 4) + 3 * sizeof(int); }
//   ccgp_cgp_predict_sets: Xs | ys | Xtests | set | params | out | state | status | res | keep
// The sets' test sites (C blocks of m x d) go up with the sets.  Per row: its m x 6 block, the 3 n + 3 doubles of its state
// that the caller may ask for (gathered on the device from its kept block, so that they come down beside `out` as one span),
// val | beta | tau2 of the state launch (res, never pulled) and the kept block itself (keep_doubles each, never pulled).
struct CgpPredictSetsStage {
  double *Xs, *ys, *Xtests;
  int* set;
  double *params, *out, *state;
  int* status;
  double *res, *keep;
  size_t nXs, nys, nXt, P, nout, nstate;
  std::vector<Piece> inputs(bool first, const double* hXs, const double* hys, const double* hXtests, const int* hset,
                            const double* hparams, int nb) const {
    return {piece(Xs, first ? hXs : nullptr, nXs), piece(ys, first ? hys : nullptr, nys),
            piece(Xtests, first ? hXtests : nullptr, nXt), piece(set, hset, (size_t)nb),
            piece(params, hparams, (size_t)nb * P)};
  }
  // the status words follow state (pull_status); hstate == nullptr: the caller does not want the states
  std::vector<Piece> results(double* hout, double* hstate, int nb) const {
    return {piece(out, hout, (size_t)nb * nout), piece(state, hstate, (size_t)nb * nstate)};
  }
};
inline CgpPredictSetsStage cgp_predict_sets_stage(Layout& c, int n, int d, int C, int m, size_t keep_doubles, int nb) {
  CgpPredictSetsStage s;
  s.nXs = (size_t)C * n * d; s.nys = (size_t)C * n; s.nXt = (size_t)C * m * d; s.P = 2 * (size_t)d + 2;
  s.nout = (size_t)m * 6; s.nstate = 3 * (size_t)n + 3;
  s.Xs = c.take<double>(s.nXs);
  s.ys = c.take<double>(s.nys);
  s.Xtests = c.take<double>(s.nXt);
  s.set = c.take<int>(nb);
  s.params = c.take<double>((size_t)nb * s.P);
  s.out = c.take<double>((size_t)nb * s.nout);
  s.state = c.take<double>((size_t)nb * s.nstate);
  s.status = c.take<int>(nb);
  s.res = c.take<double>(3 * (size_t)nb);
  s.keep = c.take<double>((size_t)nb * keep_doubles);
  return s;
}
inline size_t cgp_predict_sets_row_bytes(int n, int d, int m, size_t keep_doubles) {
  return sizeof(double) * (2 * (size_t)d + 2 + 6 * (size_t)m + 3 * (size_t)n + 3 + 3 + keep_doubles) + 2 * sizeof(int);
}

// ---- the Combined GP's and the single GP's prediction over sets (ccgp_predict_batch_sets, ccgp_krige_predict_batch_sets,
// ccgp_predict_summary_sets): per set with rows the pieces the single-set call stages, each with its alignment there, laid in
// three passes so that both copies are one span --
//   1. inputs, set by set:  X | y | params (nb x P) | Xtest | sigma2_row? | y_at?          (up)
//   2. tables, set by set:  mean | var | idx? | count?        (down without a summary; with one they never leave the device)
//   3. results, set by set: out? | beta | q? | status                                       (down)
// A set no row refers to takes nothing (every pointer null, nb 0).  off: where the set's rows start among the grouped rows.
struct SetPieces {
  int nb, off;
  double *X, *y, *Xt, *params, *s2row, *y_at;
  double *mean, *var, *out, *beta, *q;
  int *status, *idx, *count;
};
inline std::vector<SetPieces> predict_sets_stage(Layout& w, const std::vector<int>& nb_of, int n, int d, int P, int m, bool krige,
                                                 bool s2row, bool summary, bool y_at, size_t nout) {
  std::vector<SetPieces> sp(nb_of.size());
  int off = 0;
  for (size_t c = 0; c < sp.size(); ++c) {
    SetPieces& s = sp[c];
    s = SetPieces{};
    s.nb = nb_of[c];
    s.off = off;
    off += s.nb;
    if (!s.nb) continue;
    const size_t nb = (size_t)s.nb;
    s.X = w.take<double>((size_t)n * d);
    s.y = w.take<double>(n);
    s.params = w.take<double>(nb * P);
    s.Xt = w.take<double>((size_t)m * d);
    s.s2row = s2row ? w.take<double>(nb) : nullptr;
    s.y_at = y_at ? w.take<double>(m) : nullptr;
  }
  for (SetPieces& s : sp) {
    if (!s.nb) continue;
    const size_t nb = (size_t)s.nb;
    s.mean = w.take<double>(nb * m);
    s.var = w.take<double>(nb * m);
    if (summary) {
      s.idx = w.take<int>(nb);
      s.count = w.take<int>(1);
    }
  }
  for (SetPieces& s : sp) {
    if (!s.nb) continue;
    const size_t nb = (size_t)s.nb;
    if (summary) s.out = w.take<double>(nout);
    s.beta = w.take<double>(nb);
    s.q = krige ? w.take<double>(nb) : nullptr;
    s.status = w.take<int>(nb);
  }
  return sp;
}

// The same three calls on their one-launch route (small_route_predict_sets == Reg): the rows are grouped by set (a set's rows
// consecutive, in their order), so that one B x P parameter table, one set index per row and B x m tables serve every set:
//   up:    Xs | ys | sigma2_set | Xtests | set | off | nb | params | s2row? | y_at?
//   stay:  mean | var | idx? | count?          (down without a summary)
//   down:  out? | beta | q? | status
struct PredictSetsOneStage {
  double *Xs, *ys, *sigma2_set, *Xtests;
  int *set, *off, *nb;
  double *params, *s2row, *y_at, *mean, *var;
  int *idx, *count;
  double *out, *beta, *q;
  int* status;
  size_t nXs, nys, C, nXt, B, nparams, nyat, ntab, nout;
  std::vector<Piece> inputs(const double* hXs, const double* hys, const double* hs2set, const double* hXt, const int* hset,
                            const int* hoff, const int* hnb, const double* hparams, const double* hs2row,
                            const double* hyat) const {
    return {piece(Xs, hXs, nXs), piece(ys, hys, nys), piece(sigma2_set, hs2set, C), piece(Xtests, hXt, nXt), piece(set, hset, B),
            piece(off, hoff, C), piece(nb, hnb, C), piece(params, hparams, nparams), piece(s2row, hs2row, s2row ? B : 0),
            piece(y_at, hyat, y_at ? nyat : 0)};
  }
  // hmean / hvar: nullptr for a summary (the tables stay); hout: nullptr without one
  std::vector<Piece> results(double* hmean, double* hvar, double* hout, double* hbeta, double* hq, int* hstatus) const {
    return {piece(mean, hmean, hmean ? ntab : 0), piece(var, hvar, hvar ? ntab : 0), piece(out, hout, out ? nout : 0),
            piece(beta, hbeta, B), piece(q, hq, q ? B : 0), piece(status, hstatus, B)};
  }
};
inline PredictSetsOneStage predict_sets_one_stage(Layout& w, int n, int d, int P, int C, int B, int m, bool krige, bool s2row,
                                                  bool summary, bool y_at, size_t nout_per_set) {
  PredictSetsOneStage s;
  s.nXs = (size_t)C * n * d; s.nys = (size_t)C * n; s.C = C; s.nXt = (size_t)C * m * d; s.B = B; s.nparams = (size_t)B * P;
  s.nyat = (size_t)C * m; s.ntab = (size_t)B * m; s.nout = (size_t)C * nout_per_set;
  s.Xs = w.take<double>(s.nXs);
  s.ys = w.take<double>(s.nys);
  s.sigma2_set = w.take<double>(C);
  s.Xtests = w.take<double>(s.nXt);
  s.set = w.take<int>(B);
  s.off = w.take<int>(C);
  s.nb = w.take<int>(C);
  s.params = w.take<double>(s.nparams);
  s.s2row = s2row ? w.take<double>(B) : nullptr;
  s.y_at = y_at ? w.take<double>(s.nyat) : nullptr;
  s.mean = w.take<double>(s.ntab);
  s.var = w.take<double>(s.ntab);
  s.idx = summary ? w.take<int>(B) : nullptr;
  s.count = summary ? w.take<int>(C) : nullptr;
  s.out = summary ? w.take<double>(s.nout) : nullptr;
  s.beta = w.take<double>(B);
  s.q = krige ? w.take<double>(B) : nullptr;
  s.status = w.take<int>(B);
  return s;
}

// the staging ccgp_reserve(n, d, K, B, m) provides: the host-pointer likelihood and, with test sites, the prediction
// (without its tail) and the tables of ccgp_predict_summary_dev
inline size_t reserve_stage_bytes(int n, int d, int P, int B, int m) {
  size_t bytes = layout_bytes([&](Layout& c) { loglik_stage(c, n, d, P, B); });
  if (m > 0) {
    const size_t pr = layout_bytes([&](Layout& c) { predict_stage(c, n, d, P, B, m); });
    const size_t sm = layout_bytes([&](Layout& c) { summary_dev_stage(c, B, m, true); });
    bytes = bytes > pr ? bytes : pr;
    bytes = bytes > sm ? bytes : sm;
  }
  return bytes;
}

// ---- blocked sweep ---------------------------------------------------------------------------------------------------
// where a sweep leaves the likelihood, beta and status of its matrices, each indexed by draw
struct SweepOut {
  double *loglik, *beta;
  int* status;
};
// blocked prediction: scratch behind the matrices for the outputs the caller did not ask for
inline SweepOut predict_tail(Layout& t, int S, double* d_beta, int* d_status) {
  SweepOut p;
  p.loglik = t.take<double>(S);
  p.beta = d_beta ? d_beta : t.take<double>(S);
  p.status = d_status ? d_status : t.take<int>(S);
  return p;
}

}  // namespace ccgp
