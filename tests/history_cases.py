"""One table of subject calls for tests/test_gpu_handle_history.py: every batched entry point of include/ccgp.h, every
(op, route) cell of tests/route_witnesses.py, the blocked sweep's variants, the forms of the small evaluators, the two
other kernel families, the three device-pointer entry points and the two ccgp_multi calls -- each at the smallest shape
that reaches it, and each as a closure that returns EVERYTHING the call gives back: the values, the optional outputs,
status and the C return values (key "rc": one entry per checked C call the binding made).

A Subject carries the handle state its call needs (options, kernel family, workspace limit) and sets and restores it
around the call, so that any sequence of subjects can run on one handle.  Subject.call(h, fill) does, in this order:
state, `prepare` (ccgp_reserve for the device-pointer subjects), the fill (Handle.debug_fill_scratch), the call under
the timing counters, the tier check, state restored.

Inputs come from the suite's generators (conftest.synthetic_design, test_gpu_random_shapes.draws,
test_gpu_gradient_exact._design / _rows, test_gpu_design_grad._case, test_gpu_sets._sets_case,
test_gpu_marginal_exact.grid_inputs, test_gpu_cgp.rows_in_the_box, exact_designs).  Every row is well conditioned
(status 0, finite outputs); the exceptions are the four `+singular` copies, which carry exactly one singular row of an
exact design among passing ones (exact_designs: the pivot index is derived, not measured), and the streamed summary,
whose route only exists beyond 2048 draws and which carries one such row too ("with failed draws present").

Shapes: n in {1, 5, 14, 64, 100, 104, 105, 128, 129, 257} plus what a route witness needs (49, 81, 97, 101, 108) and the
n = 90 / 130 the factor-set and grid subjects are asked at; B and S from 2 to 5, 66 for the one-wave forms, 2049 for the
streamed summary.  Nothing needs more than a few MB of workspace.
"""
import functools

import numpy as np

import exact_designs as ex
import route_witnesses
from conftest import synthetic_design
from oracle import ccgp_oracle as orc
from test_gpu_design_grad import _case
from test_gpu_gradient_exact import _design, _rows, _timed
from test_gpu_random_shapes import draws

OPTION_DEFAULTS = {2: 1, 3: 1, 4: 0, 5: 0, 7: 3, 8: 11, 9: 1, 10: 1}     # include/ccgp.h: CCGP_OPT_* -> default
FUSE_DIAG, TAIL_STRIPS, WIDE_OFFSETS, SMALL_GRID16, SCHED, SCHED_POLICY, PREDICT_FACTOR, FUSED_SOLVE = 2, 3, 4, 5, 7, 8, 9, 10
GAUSS, MATERN, SPLINE = 0, 1, 2
UNLIMITED = 200 << 30            # what tests/test_gpu_failure_contract.py restores the workspace limit to
LEVELS = (0.025, 0.5, 0.975)
CELLS = {(op, r): (n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0]}


def _api():
    from ccgp_amd import api
    return api


def new_handle():
    try:
        import torch  # noqa: F401  (before libccgp is loaded: INTEGRATION.md section 5)
    except ImportError:
        pass
    return _api().Handle(0)


class Multi:
    """ccgp_multi with shards [0, 0, 0] behind the few methods Subject.call uses of a Handle."""

    def __init__(self):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.m = _api().MultiHandle([0, 0, 0])

    def _shards(self):
        from ctypes import c_void_p
        L = _api().lib()
        return [c_void_p(L.ccgp_multi_handle(self.m._m, i)) for i in range(self.m.count())]

    def debug_fill_scratch(self, byte):
        rcs = self.m.debug_fill_scratch(byte)
        assert len(rcs) == 3
        return max(rcs, key=abs)

    def workspace_bytes(self):
        from ctypes import byref, c_size_t
        ws = st = 0
        for h in self._shards():
            a, b = c_size_t(), c_size_t()
            assert _api().lib().ccgp_workspace_bytes(h, byref(a), byref(b)) == 0
            ws, st = ws + a.value, st + b.value
        return ws, st

    def close(self):
        self.m.close()


class _Spy:
    """Every C return value that passes through obj._chk inside the block."""

    def __init__(self, obj):
        self.obj, self.rcs = obj, []

    def __enter__(self):
        orig = type(self.obj)._chk.__get__(self.obj)

        def chk(rc):
            self.rcs.append(rc)
            return orig(rc)
        self.obj._chk = chk
        return self

    def __exit__(self, *exc):
        del self.obj._chk


def assert_tier(t, tier, n):
    if tier == "small":
        assert t["fused"][1] > 0 and t["update"][1] == 0 and t["diag"][1] == 0 and t["sweep"][1] == 0, t
    elif tier == "blocked":
        assert t["fused"][1] == 0 and t["sweep"][1] == 0 and t["diag"][1] > 0 and (n <= 128 or t["update"][1] > 0), t
    elif tier == "sched":
        assert t["sweep"][1] > 0 and t["fused"][1] == 0, t
    elif tier == "cov":
        assert t["cov"][1] > 0 and t["fused"][1] == 0 and t["diag"][1] == 0 and t["sweep"][1] == 0, t
    else:
        assert tier is None, tier


class Subject:
    """id; entry (the C entry point's name without ccgp_); tier in {small, blocked, sched, cov, None}; n (for the tier
    check); make() -> inputs (cached); run(h, inputs) -> dict of outputs; options ((opt, value), ...); kernel (family, nu);
    limit; prepare(h, inputs); uses_ws: the call runs in the handle's workspace; fixed_ws: workspace_bytes() must not
    change across the call; failing = {row: derived pivot} and row_keys = the float outputs with one row per draw, for the
    subjects that carry singular rows (`singular`: one of the four designated copies); multi: runs on a Multi instead of a
    Handle; cell: the (op, route) cell of route_witnesses the subject is the case of; torch: its buffers are torch tensors."""

    def __init__(self, id, entry, tier, n, make, run, options=(), kernel=None, limit=None, prepare=None, uses_ws=None,
                 fixed_ws=False, failing=None, row_keys=(), multi=False, cell=None, torch=False):
        self.id, self.entry, self.tier, self.n, self.run, self.options, self.kernel = id, entry, tier, n, run, tuple(options), kernel
        self.limit, self.prepare, self.fixed_ws, self.multi, self.cell, self.torch = limit, prepare, fixed_ws, multi, cell, torch
        self.uses_ws = tier in ("blocked", "sched") if uses_ws is None else uses_ws
        self.failing, self.row_keys = dict(failing or {}), tuple(row_keys)
        self.singular = id.endswith("+singular")
        assert not self.singular or len(self.failing) == 1
        self.inputs = functools.lru_cache(maxsize=None)(make)

    def __repr__(self):
        return self.id

    def factory(self):
        return Multi() if self.multi else new_handle()

    def call(self, h, fill=None, limit=None):
        """-> (outputs, workspace figures just before the call).  limit: a workspace limit for this call alone."""
        inp = self.inputs()
        lim = self.limit if limit is None else limit
        try:
            for opt, val in self.options:
                h.set_option(opt, val)
            if self.kernel:
                h.set_kernel(*self.kernel)
            if lim is not None:
                h.set_workspace_limit(lim)
            if self.prepare:
                self.prepare(h, inp)
            if fill is not None:
                assert h.debug_fill_scratch(fill) == 0, (self.id, fill)
            before = h.workspace_bytes()
            def spied():
                with _Spy(h.m if self.multi else h) as spy:
                    return self.run(h.m if self.multi else h, inp), spy.rcs
            (out, rcs), t = (spied(), None) if self.multi else _timed(h, spied)
            if t is not None:
                assert_tier(t, self.tier, self.n)
            if self.fixed_ws:
                assert h.workspace_bytes() == before, (self.id, before, h.workspace_bytes())
        finally:
            if not self.multi:
                for opt, _ in self.options:
                    h.set_option(opt, OPTION_DEFAULTS[opt])
                if self.kernel:
                    h.set_kernel(GAUSS, 0.0)
                if lim is not None:
                    h.set_workspace_limit(UNLIMITED)
        out = {k: np.atleast_1d(np.asarray(v)) for k, v in out.items() if v is not None}
        out["rc"] = np.asarray(rcs, dtype=np.int64)
        return out, before

    def check(self, out):
        """Passing rows are finite with status 0; the designated singular row has its derived pivot and is NaN."""
        st = out.get("status")
        bad = self.failing
        if st is not None:
            want = np.zeros(st.shape, dtype=st.dtype)
            for row, pivot in bad.items():
                want[row] = pivot
            np.testing.assert_array_equal(st, want, err_msg=self.id)
        if "code" in out:
            return
        assert (out["rc"] >= 0).all() and int(out["rc"].max(initial=0)) == len(bad), (self.id, out["rc"])
        for k, v in out.items():
            if v.dtype != np.float64:
                continue
            if k in self.row_keys:
                fail = np.zeros(v.shape[0], dtype=bool)
                fail[list(bad)] = True
                assert np.isnan(v[fail]).all() and np.isfinite(v[~fail]).all(), (self.id, k)
            else:
                assert np.isfinite(v).all(), (self.id, k)


# ----------------------------------------------------------------------------- inputs
def gauss(n, d, K, B, m=0):
    def make():
        X, y = synthetic_design(n, d, seed=n + d)
        rng = np.random.default_rng(1000 * n + 10 * d + K)
        out = dict(X=X, y=y, K=K, P=draws(rng, n, d, K, B))
        if m:
            out["Xt"] = rng.random((m, d))
            out["y_at"] = np.linspace(float(y.min()), float(y.max()), m)
        return out
    return make


def witness(n, d, K, m=0):
    """The inputs tests/test_gpu_routes.py gives the witness shapes."""
    def make():
        X, y = _design(n, d, seed=n + d)
        rng = np.random.default_rng(n)
        out = dict(X=X, y=y, K=K, P=draws(rng, n, d, K, 2))
        if m:
            out["Xt"] = rng.random((m, d))
        return out
    return make


def exact(n, seps, K, zero_sets, m=0):
    """An exact design with the separator subsets of each row; expected status derived."""
    def make():
        D = ex.ExactDesign(n, seps)
        rows, exp = D.draws(K, zero_sets)
        out = dict(X=D.X, y=D.y, K=K, P=rows, expected=exp)
        if m:
            out["Xt"] = D.sites(m, 64)[0]
            out["y_at"] = np.linspace(-1.0, 2.0, m)
        return out
    return make


def _bad(n, seps, zero_sets):
    """{row: derived pivot} of the rows that zero a separator."""
    D = ex.ExactDesign(n, seps)
    return {b: D.expected(z) for b, z in enumerate(zero_sets) if D.expected(z)}


# ----------------------------------------------------------------------------- closures, one per entry point
def r_loglik(mode=0, tau2=0.0, s2=1.3):
    def run(h, i):
        ll, beta, st = h.loglik_batch(i["X"], i["y"], i["K"], i["P"], s2, mode, tau2)
        return dict(loglik=ll, beta=beta, status=st)
    return run


def r_grad(h, i):
    ll, beta, g, st = h.loglik_grad_batch(i["X"], i["y"], i["K"], i["P"], 1.1)
    return dict(loglik=ll, beta=beta, grad=g, status=st)


def r_profile(grad):
    def run(h, i):
        ll, s2, beta, g, st = h.profile_batch(i["X"], i["y"], i["K"], i["P"], grad=grad)
        return dict(loglik=ll, sigma2=s2, beta=beta, grad=g, status=st)
    return run


def r_predict(h, i):
    mean, var, beta, st = h.predict_batch(i["X"], i["y"], i["K"], i["P"], i["Xt"], 1.3)
    return dict(mean=mean, var=var, beta=beta, status=st)


def r_krige(form):
    def run(h, i):
        s2 = None if form == 2 else 0.5 + 0.25 * np.arange(len(i["P"]))
        mean, var, beta, q, st = h.krige_predict_batch(i["X"], i["y"], i["K"], i["P"], s2, i["Xt"], form)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    return run


def r_loo(form):
    def run(h, i):
        s2 = None if form == 2 else 0.5 + 0.25 * np.arange(len(i["P"]))
        mean, var, beta, q, st = h.loo_batch(i["X"], i["y"], i["K"], i["P"], s2, form)
        return dict(mean=mean, var=var, beta=beta, q=q, status=st)
    return run


def _summary(r):
    return dict(y_hat=r["y_hat"], pred_var=r["pred_var"], quant=r["quant"], cdf_at=r["cdf_at"], quantiles=r["quantiles"],
                beta=r["beta"], status=r["status"], n_failed=np.int64(r["n_failed"]))


def r_loo_summary(h, i):
    return _summary(h.loo_summary(i["X"], i["y"], i["K"], i["P"], 1.3, LEVELS))


def r_summary(h, i):
    return _summary(h.predict_summary(i["X"], i["y"], i["K"], i["P"], i["Xt"], 1.3, LEVELS, i["y_at"]))


def r_logpost(want_Rinv, prior=1):
    def run(h, i):
        r = h.logpost(i["X"], i["y"], 1.3, prior, i["theta_t"], i.get("pars"), want_Rinv=want_Rinv)
        return dict(val=r["val"], beta=r["beta"], loglik=r["loglik"], R_inv=r["R_inv"], status=np.int32(r["status"]))
    return run


def r_logpost_batch(h, i):
    val, beta, ll, st = h.logpost_batch(i["X"], i["y"], 1.3, 0, i["theta_t"], i["pars"])
    return dict(val=val, beta=beta, loglik=ll, status=st)


def r_sets(mode, tau2):
    def run(h, i):
        ll, beta, st = h.loglik_batch_sets(i["Xs"], i["ys"], i["s2"], i["K"], i["P"], i["set"], mode, tau2)
        return dict(loglik=ll, beta=beta, status=st)
    return run


def r_logpost_sets(h, i):
    val, beta, ll, st = h.logpost_sets(i["Xs"], i["ys"], i["s2"], 2, i["theta_t"], i["set"])
    return dict(val=val, beta=beta, loglik=ll, status=st)


def r_grid(h, i):
    vals, arg, logs = h.grid_marginal(i["X"], i["y"], i["s2"], i["H"], i["N"], i["tau"], True, i["lam"], want_logs=True)
    return dict(out=vals, argmax=np.int64(arg), logs=logs)


def r_designs(h, i):
    ld, st = h.mixed_logdet_designs(i["designs"], i["K"], i["row"])
    return dict(logdet=ld, status=st)


def r_design_grad(n_fixed):
    def run(h, i):
        ld, g, st = h.mixed_logdet_grad_designs(i["designs"], i["K"], i["row"], n_fixed)
        return dict(logdet=ld, grad=g, status=st)
    return run


def r_design_grad_refused(h, i):
    try:
        h.mixed_logdet_grad_designs(i["designs"], i["K"], i["row"], 0)
    except _api().CcgpError as e:
        return dict(code=np.int64(e.code))
    raise AssertionError("the design gradient beyond its evaluator was not refused")


def r_cgp_state(h, i):
    val, beta, tau2, loo, st = h.cgp_state_batch(i["Xs"], i["y"], i["rows"], skip=i["skip"])
    return dict(val=val, beta=beta, tau2=tau2, loo=loo, status=st)


def r_cgp_predict(h, i):
    out, keep, st = h.cgp_predict(i["Xs"], i["y"], i["rows"][0], i["Xt"])
    assert keep is not None
    return dict(out=out, s=keep["s"], res2=keep["res2"], temp=keep["temp"], sf=keep["sf"], beta=keep["beta"],
                tau2=keep["tau2"], status=np.int32(st))


def r_factorset(h, i):
    with h.factor_batch(i["X"], i["y"], i["K"], i["P"], 1.3) as fs:
        nbytes = fs.nbytes
        mean, var = fs.predict(i["Xt"])
        s = fs.summary(i["Xt"], LEVELS, y_at=i["y_at"])
    assert nbytes > 0
    return dict(loglik=fs.loglik, beta=fs.beta, status=fs.status, mean=mean, var=var, y_hat=s["y_hat"], pred_var=s["pred_var"],
                quant=s["quant"], cdf_at=s["cdf_at"], quantiles=s["quantiles"], n_failed=np.int64(s["n_failed"]))


def r_corr(h, i):
    K, row = i["K"], i["P"][0]
    th = row[K:K + i["X"].shape[1]]
    return dict(R=h.corr_matrix(i["X"], th), r=h.corr_cross(i["Xt"], i["X"], th),
                Rm=h.mixed_corr_matrix(i["X"], K, row), rm=h.mixed_corr_cross(i["Xt"], i["X"], K, row))


def r_rinv(h, i):
    beta = h.beta_mle(i["R_inv"], i["y"])
    f = h.factors(i["R_inv"], i["b"], i["y"])
    mean, var = h.predict_from_factors(i["r"], i["b"], i["mf"], i["v1"], i["v2"], i["R_inv"], 1.3)
    pm, pv = h.predict_post(i["Xt"], i["X"], i["K"], i["P"][0], i["b"], i["mf"], i["v1"], i["v2"], i["R_inv"], 1.3)
    return dict(beta=beta, sigma2=h.sigma2_mle(i["R_inv"], i["y"], i["b"]), factors=f, mean=mean, var=var, post_mean=pm,
                post_var=pv)


def with_rinv(make):
    def made():
        i = dict(make())
        K, d = i["K"], i["X"].shape[1]
        w, Th = orc.unpack_params(i["P"][0], K, d)
        i["R_inv"] = orc.solve_inverse(orc.mixed_corr_matrix_general(i["X"], w, Th))
        i["b"] = orc.beta_mle(i["R_inv"], i["y"])
        i["mf"], i["v1"], i["v2"] = orc.factors(i["R_inv"], i["b"], i["y"])
        i["r"] = np.stack([orc.mixed_corr_vec_general(x, i["X"], w, Th) for x in i["Xt"]])
        return i
    return made


def iso(n, d, B, prior_pars=None):
    """Transformed parameter vectors (log theta1, log theta2, logit p) of well-conditioned isotropic draws."""
    def make():
        X, y = _design(n, d, seed=6000 + n)
        rough = 2.0 * n ** (2.0 / d) / d
        rng = np.random.default_rng(n + d)
        p, t1, t2 = rng.uniform(0.3, 0.8, B), rng.uniform(0.2, 0.4, B) * rough, rng.uniform(1.2, 1.8, B) * rough
        th = np.column_stack([np.log(t1), np.log(t2), np.log(p / (1.0 - p))])
        return dict(X=X, y=y, theta_t=th if B > 1 else th[0], pars=prior_pars)
    return make


def sets(n, d, K, C, B, transformed=False):
    def make():
        from test_gpu_sets import _sets_case
        Xs, ys, s2, P, set_of = _sets_case(n, d, K, C, B, 100 + n)
        out = dict(Xs=Xs, ys=ys, s2=s2, K=K, P=P, set=set_of)
        if transformed:
            out["theta_t"] = iso(n, d, B)()["theta_t"]
        return out
    return make


def grid(n, d, lam, G, N, kind):
    def make():
        from test_gpu_marginal_exact import grid_inputs
        X, y, H = grid_inputs(n, d, lam, 50.0, 30.0, G, N, kind, 1.0)
        return dict(X=X, y=y, H=H, N=N, s2=30.0, tau=50.0, lam=lam)
    return make


def designs(n, d, K, B=2):
    def make():
        rng = np.random.default_rng(n)
        X, row = _case(rng, n, d, K)
        return dict(designs=np.stack([X] + [_case(rng, n, d, K)[0] for _ in range(B - 1)]), K=K, row=row)
    return make


def logdet_witness(n, d, K):
    def make():
        return dict(designs=np.stack([_design(n, d, seed=n + i)[0] for i in range(2)]), K=K,
                    row=draws(np.random.default_rng(n), n, d, K, 1)[0])
    return make


def grad_witness(n, d, K):
    def make():
        X, y = _design(n, d, seed=2000 + n + d)
        return dict(X=X, y=y, K=K, P=_rows(X, K, d, 2, seed=n + d + K))
    return make


def cgp_case(n, d, B, m):
    def make():
        from ccgp_amd import cgp
        from test_gpu_cgp import rows_in_the_box
        X, y = synthetic_design(n, d, 1000 + 10 * n + d)
        Xs, _ = cgp.standardise(X)
        return dict(Xs=Xs, y=y, rows=rows_in_the_box(Xs, B, 7 * n + d), skip=np.array([0, n - 1, n // 2, 1][:B], dtype=np.int32),
                    Xt=np.random.default_rng(n + d).random((m, d)))
    return make


def family(n, spline, B, m):
    """The 1-D families as tests/test_gpu_routes.test_matern_goes_blocked draws them."""
    def make():
        rng = np.random.default_rng(n)
        x = np.sort((np.arange(n) + rng.uniform(0.2, 0.8, n)) / n)[:, None]
        y = np.sin(9.0 * x[:, 0]) + 0.3 * np.cos(31.0 * x[:, 0])
        P = np.column_stack([rng.uniform(0.3, 0.9, B), rng.uniform(0.1, 0.7, B), rng.uniform(1.5, 3.0, B) / n,
                             rng.uniform(0.3, 0.8, B) / n * (8.0 if spline else 1.0)])
        return dict(X=x, y=y, K=2, P=P, Xt=rng.random((m, 1)), y_at=np.linspace(-1.0, 1.0, m))
    return make


def streamed_summary():
    """S = 2049 > kSummaryLdsDraws draws on an exact design of n = 14: the passing rows vary in their weights and base-dimension
    length scales and keep every separator apart; row 1000 zeroes separator 1 and fails at pivot 8."""
    def make():
        D = ex.ExactDesign(14, (2, 8, 14))
        rng = np.random.default_rng(14)
        S = 2049
        P = np.empty((S, 2 + 2 * D.d))
        for s in range(S):
            p = rng.uniform(0.2, 0.8)
            th = np.stack([np.concatenate([np.full(2, rng.uniform(0.3, 1.0)), np.full(3, ex.THETA[0])]),
                           np.concatenate([np.full(2, rng.uniform(1.5, 3.0)), np.full(3, ex.THETA[1])])])
            P[s] = np.concatenate([[p, 1.0 - p], th.ravel()])
        P[1000] = D.row(2, (1,))
        return dict(X=D.X, y=D.y, K=2, P=P, Xt=D.sites(5, 64)[0], y_at=np.linspace(-1.0, 2.0, 5))
    return make


# ----------------------------------------------------------------------------- the device-pointer entry points
def dev_subject(case):
    """One of tests/test_gpu_stream_contract.py's cases on the handle's own stream: reserve, (fill), the _dev call."""
    import test_gpu_stream_contract as sc
    c = case(sc)

    def make():
        import torch
        host, true, live = sc.problem(torch, c)
        outs, _ = sc.output_tensors(torch, c)
        return dict(true=true, live=live, outs=outs)

    def prepare(h, i):
        h.reserve(c.n, c.d, c.K, c.B, c.m)

    def run(h, i):
        import torch
        for k in i["live"]:
            i["live"][k].copy_(i["true"][k])
        for v in i["outs"].values():
            v.fill_(sc.SENTINEL if v.dtype == torch.float64 else sc.SENTINEL_INT)
        torch.cuda.synchronize()
        sc.dev_call(h, c, i["live"], i["outs"])
        h.synchronize()
        return {k: v.cpu().numpy() for k, v in i["outs"].items()}

    tier = {"small": "small", "blocked": "blocked"}[c.tier]
    return Subject("dev:" + c.id, c.entry + "_dev", tier, c.n, make, run, options=c.options, prepare=prepare, fixed_ws=True,
                   uses_ws=c.kept or tier == "blocked", torch=True)


# ----------------------------------------------------------------------------- the table
def _sweep_variants():
    out = []
    for n, d in ((257, 3), (129, 2)):
        for tag, tier, opts in (("sched0", "blocked", ((SCHED, 0),)), ("sched1", "sched", ((SCHED, 1),)),
                                ("sched2", "sched", ((SCHED, 2),)), ("fused-solve0", "blocked", ((FUSED_SOLVE, 0),)),
                                ("fused-solve2", "blocked", ((FUSED_SOLVE, 2),)), ("fuse-diag0", "blocked", ((FUSE_DIAG, 0),)),
                                ("fuse-diag1", "blocked", ((FUSE_DIAG, 1),)), ("tail-strips0", "blocked", ((TAIL_STRIPS, 0),)),
                                ("tail-strips1", "blocked", ((TAIL_STRIPS, 1),)), ("wide-offsets1", "blocked", ((WIDE_OFFSETS, 1),))):
            out.append(Subject("sweep-n%d-%s" % (n, tag), "loglik_batch", tier, n, gauss(n, d, 2, 3), r_loglik(), options=opts))
    return out


def _singular():
    z129, z64, z257 = [(), (1,), (), ()], [(), (), (1,), ()], [(), (2,), ()]
    s129, s64, s257 = ex.LOGLIK_BLOCKED[129], ex.predict_seps(64), ex.GRAD_BLOCKED_SEPS
    return [
        Subject("loglik-blocked-n129+singular", "loglik_batch", "blocked", 129, exact(129, s129, 2, z129), r_loglik(),
                failing=_bad(129, s129, z129), row_keys=("loglik", "beta")),
        Subject("predict-kept-n64+singular", "predict_batch", "small", 64, exact(64, s64, 2, z64, m=5), r_predict, uses_ws=True,
                failing=_bad(64, s64, z64), row_keys=("mean", "var", "beta")),
        Subject("grad-blocked-n257+singular", "loglik_grad_batch", "blocked", 257, exact(257, s257, 2, z257), r_grad,
                failing=_bad(257, s257, z257), row_keys=("loglik", "beta", "grad")),
        Subject("summary-staged-n64+singular", "predict_summary", "small", 64, exact(64, s64, 2, z64, m=5), r_summary,
                uses_ws=True, failing=_bad(64, s64, z64), row_keys=("beta",)),
    ]


def _cells():
    w = CELLS
    th = iso
    return [
        Subject("cell-loglik-r", "loglik_batch", "small", 1, witness(*w["loglik", "r"]), r_loglik(), cell=("loglik", "r")),
        Subject("cell-loglik-b", "loglik_batch", "blocked", 129, witness(*w["loglik", "b"]), r_loglik(), cell=("loglik", "b")),
        Subject("cell-predict-r", "predict_batch", "small", 1, witness(*w["predict", "r"], m=3), r_predict, cell=("predict", "r")),
        Subject("cell-predict-b", "predict_batch", "blocked", 108, witness(*w["predict", "b"], m=3), r_predict,
                cell=("predict", "b")),
        Subject("cell-reserve-b", "predict_batch", "blocked", 108, witness(*w["reserve", "b"], m=3), r_predict,
                prepare=lambda h, i: h.reserve(*(w["reserve", "b"] + (2, 3))), fixed_ws=True, cell=("reserve", "b")),
        Subject("cell-grad-r", "loglik_grad_batch", "small", 1, grad_witness(*w["grad", "r"]), r_grad, cell=("grad", "r")),
        Subject("cell-grad-l", "loglik_grad_batch", "small", 97, grad_witness(*w["grad", "l"]), r_grad, cell=("grad", "l")),
        Subject("cell-grad-b", "loglik_grad_batch", "blocked", 108, grad_witness(*w["grad", "b"]), r_grad, cell=("grad", "b")),
        Subject("cell-logdet-designs-r", "mixed_logdet_designs", "small", 1, logdet_witness(*w["logdet_designs", "r"]), r_designs,
                cell=("logdet_designs", "r")),
        Subject("cell-logdet-designs-b", "mixed_logdet_designs", "blocked", 49, logdet_witness(*w["logdet_designs", "b"]),
                r_designs, cell=("logdet_designs", "b")),
        Subject("cell-design-grad-r", "mixed_logdet_grad_designs", "small", 1, designs(*w["design_grad", "r"]), r_design_grad(0),
                cell=("design_grad", "r")),
        Subject("cell-design-grad-u", "mixed_logdet_grad_designs", None, 81, designs(*w["design_grad", "u"]),
                r_design_grad_refused, cell=("design_grad", "u")),
        Subject("cell-inverse-r", "logpost", "small", 1, th(*w["inverse", "r"][:2], 1), r_logpost(True), cell=("inverse", "r")),
        Subject("cell-inverse-l", "logpost", "small", 101, th(*w["inverse", "l"][:2], 1), r_logpost(True), cell=("inverse", "l")),
        Subject("cell-inverse-b", "logpost", "blocked", 108, th(*w["inverse", "b"][:2], 1), r_logpost(True), cell=("inverse", "b")),
    ]


def _entries():
    S = Subject
    pars = np.array([7.0, 3.0, 3.0, 28.0])
    out = [
        # the small evaluators: four waves per matrix (B = 2), one wave per matrix (B = 66), the 16 x 16 grid by option
        S("loglik-n5-mode0", "loglik_batch", "small", 5, gauss(5, 2, 2, 2), r_loglik()),
        S("loglik-n5-mode1", "loglik_batch", "small", 5, gauss(5, 2, 2, 2), r_loglik(1, 25.0)),
        S("loglik-n64-B2", "loglik_batch", "small", 64, gauss(64, 3, 2, 2), r_loglik()),
        S("loglik-n64-B66", "loglik_batch", "small", 64, gauss(64, 3, 2, 66), r_loglik()),
        S("loglik-n100-B2", "loglik_batch", "small", 100, gauss(100, 3, 2, 2), r_loglik()),
        S("loglik-n100-B66-mode1", "loglik_batch", "small", 100, gauss(100, 3, 2, 66), r_loglik(1, 25.0)),
        S("loglik-n100-B66-grid16", "loglik_batch", "small", 100, gauss(100, 3, 2, 66), r_loglik(), options=((SMALL_GRID16, 1),)),
        S("loglik-n104-B66", "loglik_batch", "small", 104, gauss(104, 3, 2, 66), r_loglik()),
        S("loglik-n105-B3", "loglik_batch", "small", 105, gauss(105, 3, 2, 3), r_loglik()),
        S("loglik-n128-B3", "loglik_batch", "small", 128, gauss(128, 3, 3, 3), r_loglik(1, 25.0)),
        S("loglik-n129-mode1", "loglik_batch", "blocked", 129, gauss(129, 2, 2, 3), r_loglik(1, 25.0)),
        S("loglik-n257-chunks", "loglik_batch", "blocked", 257, gauss(257, 3, 2, 5), r_loglik(), limit=4 << 20),
        S("grad-n14", "loglik_grad_batch", "small", 14, gauss(14, 2, 2, 3), r_grad),
        S("grad-n257", "loglik_grad_batch", "blocked", 257, gauss(257, 3, 2, 2), r_grad),
        S("grad-n129-sched1", "loglik_grad_batch", "sched", 129, gauss(129, 2, 2, 2), r_grad, options=((SCHED, 1),)),
        S("profile-n64", "profile_batch", "small", 64, gauss(64, 3, 2, 3), r_profile(False)),
        S("profile-n64-grad", "profile_batch", "small", 64, gauss(64, 3, 2, 3), r_profile(True)),
        S("profile-n129", "profile_batch", "blocked", 129, gauss(129, 2, 2, 2), r_profile(False)),
        S("profile-n129-grad", "profile_batch", "blocked", 129, gauss(129, 2, 2, 2), r_profile(True)),
        S("predict-kept-n64", "predict_batch", "small", 64, gauss(64, 3, 2, 3, m=5), r_predict, uses_ws=True),
        S("predict-kept-n100-S66", "predict_batch", "small", 100, gauss(100, 3, 2, 66, m=65), r_predict, uses_ws=True),
        S("predict-extra-rows-n64-m31", "predict_batch", "small", 64, gauss(64, 3, 2, 3, m=31), r_predict,
          options=((PREDICT_FACTOR, 0),)),
        S("predict-extra-rows-n128-m63", "predict_batch", "small", 128, gauss(128, 3, 2, 3, m=63), r_predict,
          options=((PREDICT_FACTOR, 0),)),
        S("predict-blocked-n129-m3", "predict_batch", "blocked", 129, gauss(129, 2, 2, 3, m=3), r_predict),
        S("predict-blocked-n129-m129", "predict_batch", "blocked", 129, gauss(129, 2, 2, 2, m=129), r_predict),
        S("predict-blocked-n257-m3", "predict_batch", "blocked", 257, gauss(257, 3, 2, 2, m=3), r_predict),
        S("predict-blocked-n129-m3-sched1", "predict_batch", "sched", 129, gauss(129, 2, 2, 3, m=3), r_predict,
          options=((SCHED, 1),)),
        S("krige-ordinary-n64", "krige_predict_batch", "small", 64, gauss(64, 3, 2, 3, m=5), r_krige(0), uses_ws=True),
        S("krige-plugin-n64", "krige_predict_batch", "small", 64, gauss(64, 3, 2, 3, m=5), r_krige(1), uses_ws=True),
        S("krige-unbiased-n64", "krige_predict_batch", "small", 64, gauss(64, 3, 2, 3, m=5), r_krige(2), uses_ws=True),
        S("krige-unbiased-n129", "krige_predict_batch", "blocked", 129, gauss(129, 2, 2, 2, m=3), r_krige(2)),
        S("loo-n14", "loo_batch", "small", 14, gauss(14, 2, 2, 3), r_loo(0)),
        S("loo-n129-unbiased", "loo_batch", "blocked", 129, gauss(129, 2, 2, 2), r_loo(2)),
        S("loo-n257-plugin", "loo_batch", "blocked", 257, gauss(257, 3, 2, 2), r_loo(1)),
        S("loo-summary-n14", "loo_summary", "small", 14, gauss(14, 2, 2, 4), r_loo_summary),
        S("loo-summary-n129", "loo_summary", "blocked", 129, gauss(129, 2, 2, 3), r_loo_summary),
        S("summary-staged-n64", "predict_summary", "small", 64, gauss(64, 3, 2, 5, m=5), r_summary, uses_ws=True),
        S("summary-staged-n129", "predict_summary", "blocked", 129, gauss(129, 2, 2, 3, m=3), r_summary),
        S("summary-streamed-n14-S2049", "predict_summary", "small", 14, streamed_summary(), r_summary, uses_ws=True,
          limit=2 << 20, failing={1000: 8}, row_keys=("beta",)),
        S("logpost-n14", "logpost", "small", 14, iso(14, 2, 1), r_logpost(False)),
        S("logpost-rinv-n64", "logpost", "small", 64, iso(64, 3, 1, pars), r_logpost(True, 0)),
        S("logpost-rinv-n129", "logpost", "blocked", 129, iso(129, 2, 1), r_logpost(True)),
        S("logpost-n129", "logpost", "blocked", 129, iso(129, 2, 1), r_logpost(False)),
        S("logpost-batch-n14", "logpost_batch", "small", 14, iso(14, 2, 3, pars), r_logpost_batch),
        S("logpost-batch-n129", "logpost_batch", "blocked", 129, iso(129, 2, 2, pars), r_logpost_batch),
        S("sets-one-launch-n14", "loglik_batch_sets", "small", 14, sets(14, 2, 2, 3, 5), r_sets(0, 0.0)),
        S("sets-one-launch-n100-mode1", "loglik_batch_sets", "small", 100, sets(100, 2, 2, 3, 5), r_sets(1, 0.5)),
        S("sets-by-set-n129", "loglik_batch_sets", "blocked", 129, sets(129, 3, 2, 2, 3), r_sets(0, 0.0)),
        S("logpost-sets-one-launch-n14", "logpost_sets", "small", 14, sets(14, 2, 2, 3, 5, True), r_logpost_sets),
        S("logpost-sets-by-set-n129", "logpost_sets", "blocked", 129, sets(129, 3, 2, 2, 3, True), r_logpost_sets),
        S("grid-iso-shared-n14", "grid_marginal", "small", 14, grid(14, 2, -1.0, 5, 13, "shared"), r_grid),
        S("grid-aniso-shared-n14", "grid_marginal", "small", 14, grid(14, 2, 0.5, 5, 13, "shared"), r_grid),
        S("grid-iso-shared-n130", "grid_marginal", "blocked", 130, grid(130, 3, -1.0, 3, 2, "shared"), r_grid),
        S("grid-aniso-distinct-n130", "grid_marginal", "blocked", 130, grid(130, 2, 0.5, 2, 2, "distinct"), r_grid),
        S("logdet-designs-n14", "mixed_logdet_designs", "small", 14, designs(14, 2, 2, 3), r_designs),
        S("logdet-designs-n129", "mixed_logdet_designs", "blocked", 129, designs(129, 2, 2, 2), r_designs),
        S("design-grad-n14-fixed5", "mixed_logdet_grad_designs", "small", 14, designs(14, 2, 2, 3), r_design_grad(5)),
        S("cgp-state-skip-n14", "cgp_state_batch", "small", 14, cgp_case(14, 2, 4, 5), r_cgp_state, uses_ws=True),
        S("cgp-state-skip-n128", "cgp_state_batch", "small", 128, cgp_case(128, 2, 2, 5), r_cgp_state, uses_ws=True),
        S("cgp-predict-n14", "cgp_predict", "small", 14, cgp_case(14, 2, 2, 5), r_cgp_predict, uses_ws=True),
        S("cgp-predict-n100", "cgp_predict", "small", 100, cgp_case(100, 2, 2, 65), r_cgp_predict, uses_ws=True),
        S("factorset-n90", "factor_batch", "small", 90, gauss(90, 3, 2, 3, m=5), r_factorset, uses_ws=True),
        S("factorset-n257", "factor_batch", "blocked", 257, gauss(257, 3, 2, 3, m=5), r_factorset),
        S("factorset-n257-m129", "factor_batch", "blocked", 257, gauss(257, 3, 2, 2, m=129), r_factorset),
        S("corr-n100-m70", "corr_matrix", "cov", 100, gauss(100, 3, 2, 1, m=70), r_corr),
        S("corr-n129-m5", "corr_matrix", "cov", 129, gauss(129, 2, 2, 1, m=5), r_corr),
        S("rinv-helpers-n14", "beta_mle", "cov", 14, with_rinv(gauss(14, 2, 2, 1, m=5)), r_rinv),
        S("rinv-helpers-n100", "beta_mle", "cov", 100, with_rinv(gauss(100, 3, 2, 1, m=5)), r_rinv),
        # the 1-D families exist on the sweep only
        S("matern-loglik-n14", "loglik_batch", "blocked", 14, family(14, False, 3, 3), r_loglik(), kernel=(MATERN, 2.5)),
        S("matern-predict-n129", "predict_batch", "blocked", 129, family(129, False, 2, 3), r_predict, kernel=(MATERN, 2.5)),
        S("spline-predict-n14", "predict_batch", "blocked", 14, family(14, True, 3, 3), r_predict, kernel=(SPLINE, 2.5)),
        S("spline-loo-n14", "loo_batch", "blocked", 14, family(14, True, 2, 3), r_loo(0), kernel=(SPLINE, 2.5)),
    ]
    return out


def _dev_and_multi():
    def run_multi_loglik(m, i):
        ll, beta, st = m.loglik_batch(i["X"], i["y"], i["K"], i["P"], 1.3)
        return dict(loglik=ll, beta=beta, status=st)

    def run_multi_predict(m, i):
        mean, var, beta, st = m.predict_batch(i["X"], i["y"], i["K"], i["P"], i["Xt"], 1.3)
        return dict(mean=mean, var=var, beta=beta, status=st)

    return [
        dev_subject(lambda sc: sc.Case("loglik", 129, 2, 2, 2, tier="blocked")),
        dev_subject(lambda sc: sc.Case("loglik", 64, 3, 2, 66, mode=1, tag="grid8x8")),
        dev_subject(lambda sc: sc.Case("predict", 14, 2, 2, 5, m=65, kept=True)),
        dev_subject(lambda sc: sc.Case("predict", 130, 3, 2, 4, m=3, tier="blocked")),
        dev_subject(lambda sc: sc.Case("summary", 14, 2, 2, 5, m=5, kept=True, tag="all-buffers")),
        dev_subject(lambda sc: sc.Case("summary", 130, 3, 2, 4, m=3, tier="blocked")),
        Subject("multi-loglik-n129", "multi_loglik_batch", None, 129, gauss(129, 2, 2, 5), run_multi_loglik, multi=True,
                uses_ws=True),
        Subject("multi-predict-n64", "multi_predict_batch", None, 64, gauss(64, 3, 2, 5, m=5), run_multi_predict, multi=True,
                uses_ws=True),
    ]


@functools.lru_cache(maxsize=None)
def table():
    subjects = _cells() + _entries() + _sweep_variants() + _singular() + _dev_and_multi()
    ids = [s.id for s in subjects]
    assert len(set(ids)) == len(ids)
    return tuple(subjects)


# Not in the table: what a natural history puts in front of a subject.  A batch whose every row fails (before the same
# shape's passing batch), on the sweep and on the register evaluator.
def interludes():
    all129 = [(0,), (1,), (2,)]
    all64 = [(0,), (1,), (2, 0)]
    return {
        "all-fail-blocked-n129": Subject("all-fail-blocked-n129", "loglik_batch", "blocked", 129,
                                         exact(129, ex.LOGLIK_BLOCKED[129], 2, all129), r_loglik(),
                                         failing=_bad(129, ex.LOGLIK_BLOCKED[129], all129), row_keys=("loglik", "beta")),
        "all-fail-kept-n64": Subject("all-fail-kept-n64", "predict_batch", "small", 64,
                                     exact(64, ex.predict_seps(64), 2, all64, m=5), r_predict, uses_ws=True,
                                     failing=_bad(64, ex.predict_seps(64), all64), row_keys=("mean", "var", "beta")),
    }


ENTRY_POINTS = ("loglik_batch", "loglik_grad_batch", "profile_batch", "predict_batch", "krige_predict_batch", "loo_batch",
                "loo_summary", "predict_summary", "logpost", "logpost_batch", "loglik_batch_sets", "logpost_sets",
                "grid_marginal", "mixed_logdet_designs", "mixed_logdet_grad_designs", "cgp_state_batch", "cgp_predict",
                "factor_batch", "corr_matrix", "beta_mle", "loglik_dev", "predict_dev", "summary_dev", "multi_loglik_batch",
                "multi_predict_batch")
