"""The stream contract of the device-pointer entry points (include/ccgp.h): ccgp_loglik_batch_dev, ccgp_predict_batch_dev
and ccgp_predict_summary_dev "only enqueue work on the handle's stream", with "no allocation, no synchronisation once the
workspace has been sized by ccgp_reserve", on a caller-owned stream after ccgp_set_stream.

Every case runs ONE staged call (staged_call below) on a caller-owned torch stream, on a fresh handle that has been
reserved for exactly that shape, with no host synchronisation between the first and the last enqueue:

    inputs = NaN, outputs = sentinel | delay | inputs <- true values | the _dev call | snapshots <- outputs | inputs = NaN

* A library that runs on another stream, forks its second stream (kept-factor prediction: csrc/small_reg.hip,
  launch_small_reg_predict) from the wrong point or does not join it back reads the NaN, or leaves the sentinel in the
  snapshot: the snapshot then differs from the reference.
* A library that synchronises returns only after the delay: the event recorded behind the delay has completed.
* A library that allocates changes Handle.workspace_bytes() (and, for scratch of 64 MiB and more, the device's free
  memory).

Reference: the host-pointer entry point of the same shape on the same handle, called afterwards; the suite holds its values
to the long-double references (test_gpu_marginal_exact, test_gpu_predict_exact, test_gpu_predict_summary) and host = dev
bit for bit on the handle's own stream.  Here every output must have its bits: no tolerance.

Every detector is one deterministic run and one-sided.  The delay is a chain of fp64 matmuls on the stream under test,
calibrated once to at least 50 ms (printed; measured 51.2 ms with 27 products of 4096 x 4096) against a host
enqueue of 70 us (one logpost round trip) to about a millisecond (a hundred launches of a sweep at n = 385): a delay that is
too short makes a case FAIL.  A join that is missing but whose second stream happened to finish first is not seen: a
passing run proves the order that was enqueued, not the absence of a race; nothing here is repeated to look for one.

Before the staged call a second, throw-away handle runs the same call once on the same stream: code objects load and
queues get their scratch on a kernel's first launch in the process, which is the runtime's business and not the handle's.
The handle under test stays fresh: it has only been created, configured and reserved.

The whole module takes 5 s on an MI355X: 0.06 s per case (one delay plus milliseconds), 2 s to load torch and calibrate.
"""
import math
import os

import numpy as np
import pytest

import route_witnesses
from conftest import ROOT, load_maximin, synthetic_design
from test_gpu_gradient_exact import _timed
from test_gpu_marginal_exact import CHUNK_CASE, SCHED_CASE
from test_gpu_random_shapes import draws

pytestmark = pytest.mark.gpu

DELAY_MS = 50.0
SENTINEL, SENTINEL_INT = -777.25, -7
LEVELS = (1e-9, 0.025, 0.5, 0.975, 1.0 - 1e-9)
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")


# ----------------------------------------------------------------------------- layout of the kept-factor scratch
def fac_npf(n):
    return (n + 7) // 8 * 8


def fac_total(n):
    """csrc/small_layout.h FacLayout(n).total, in doubles: hdr[8] | rd | zy | z1 (npf each) | L' packed, padded to 8."""
    return (8 + 3 * fac_npf(n) + n * (n - 1) // 2 + 7) // 8 * 8


def sites_scratch(n, m):
    """csrc/small_layout.h small_reg_sites_scratch: bytes per draw, the factor block and ceil(m / 64) batches of 64 sites."""
    return 8 * (fac_total(n) + (m + 63) // 64 * fac_npf(n) * 64)


def kept_ws(n, m, S, limit=None):
    """csrc/capi.hip kept_factor_ws_bytes: all S draws, or as many as half the workspace limit holds (at least 64)."""
    per = sites_scratch(n, m)
    if limit is None:
        return per * S
    return min(per * S, max(limit // 2, per * 64) // per * per)


def test_layout_mirror_matches_the_headers():
    """The three functions above against the text they mirror (as test_gpu_predict_summary.lds_cap reads its constant)."""
    lay = open(os.path.join(CSRC, "small_layout.h")).read()
    assert "CCGP_HD constexpr int fac_npf(int n) { return (n + 7) / 8 * 8; }" in lay
    assert "rd = 8; zy = rd + npf; z1 = zy + npf; L = z1 + npf; head = L; total = (L + n * (n - 1) / 2 + 7) / 8 * 8;" in lay
    assert "return sizeof(double) * ((size_t)FacLayout(n).total + (size_t)((m + 63) / 64) * fac_npf(n) * 64);" in lay
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert "const size_t want = per * (size_t)S, cap = std::max<size_t>(h->ws_limit / 2, per * 64);" in capi
    assert "return std::min(want, cap / per * per);" in capi
    assert kept_ws(100, 5, 1000) >= 64 << 20 > kept_ws(100, 5, 300)


# ----------------------------------------------------------------------------- the delay
class Delay:
    """A chain of fp64 products I @ x on the current stream; `count` is fixed once, where the chain alone measures >= 50 ms."""

    def __init__(self, torch, stream):
        self.torch = torch
        dev = torch.device("cuda:0")
        self.eye = torch.eye(4096, dtype=torch.float64, device=dev)
        self.x = torch.rand(4096, 4096, dtype=torch.float64, device=dev)
        self.y = torch.empty_like(self.x)
        self.count = 4
        self.measure(stream)                       # first launches: library initialisation, not the chain
        while True:
            self.ms = self.measure(stream)
            if self.ms >= DELAY_MS:
                break
            self.count = max(self.count + 1, int(math.ceil(self.count * 1.1 * DELAY_MS / self.ms)))
        print("delay: %d products of 4096 x 4096 fp64 = %.1f ms" % (self.count, self.ms))

    def run(self):
        a, b = self.x, self.y
        for _ in range(self.count):
            self.torch.mm(self.eye, a, out=b)
            a, b = b, a

    def measure(self, stream):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            e0.record()
            self.run()
            e1.record()
        stream.synchronize()
        return e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def torch():
    import torch                                  # before libccgp is loaded
    return torch


@pytest.fixture(scope="module")
def stream(torch):
    return torch.cuda.Stream()


@pytest.fixture(scope="module")
def delay(torch, stream):
    return Delay(torch, stream)


# ----------------------------------------------------------------------------- the staged call
def staged_call(torch, stream, delay, call, inputs, outputs):
    """inputs: (live, true) pairs of device tensors -- `call` reads the live ones; outputs: (out, snapshot) pairs.  Everything
    goes onto `stream`; the host waits once, at the end.  Returns whether the event behind the delay was still pending when
    `call` returned (asserted by the caller AFTER the stream has drained, so that a failure leaves nothing in flight)."""
    nan = float("nan")
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for live, _ in inputs:
            live.fill_(nan)
        for out, snap in outputs:
            sentinel = SENTINEL if out.dtype == torch.float64 else SENTINEL_INT
            out.fill_(sentinel)
            snap.fill_(sentinel)
        delay.run()
        ev.record(stream)
        for live, true in inputs:
            live.copy_(true)
        call()
        pending = not ev.query()
        for out, snap in outputs:
            snap.copy_(out)
        for live, _ in inputs:
            live.fill_(nan)
    stream.synchronize()
    return pending


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ----------------------------------------------------------------------------- cases
class Case:
    """One call: entry in {loglik, predict, summary}; B = draws; tier in {small, blocked, sched, chunks}; kept = the
    kept-factor scheme serves it (its scratch is then the whole workspace)."""

    def __init__(self, entry, n, d, K, B, m=0, mode=0, tier="small", kept=False, options=(), limit=None, matern=False,
                 optional=True, tag=""):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.id = "%s-n%d-d%d-K%d-B%d%s%s%s" % (entry, n, d, K, B, "-m%d" % m if m else "",
                                                 "-mode%d" % mode if entry == "loglik" else "", "-" + tag if tag else "")


def _api():
    from ccgp_amd import api
    return api


def loglik_cases():
    api = _api()
    out = []
    for mode in (0, 1):
        out += [Case("loglik", 5, 2, 2, 2, mode=mode, tag="grid16x16"),
                Case("loglik", 64, 3, 2, 66, mode=mode, tag="grid8x8"),
                Case("loglik", 72, 3, 2, 66, mode=mode, tag="one-wave"),
                Case("loglik", 105, 3, 2, 2, mode=mode),
                Case("loglik", 129, 2, 2, 2, mode=mode, tier="blocked"),
                Case("loglik", *SCHED_CASE, mode=mode, tier="sched", options=((api.OPT_SCHED, 1),), tag="sched1"),
                Case("loglik", *SCHED_CASE, mode=mode, tier="sched", options=((api.OPT_SCHED, 2),), tag="sched2"),
                Case("loglik", *CHUNK_CASE, mode=mode, tier="chunks", limit=8 << 20, tag="chunks")]
    return out


def predict_cases():
    api = _api()
    return [Case("predict", 14, 2, 2, 300, m=65, kept=True),
            Case("predict", 100, 3, 2, 300, m=5, kept=True),
            Case("predict", 50, 3, 2, 200, m=5, kept=True, limit=1 << 20, tag="chunks-of-64"),
            Case("predict", 14, 2, 2, 300, m=65, options=((api.OPT_PREDICT_FACTOR, 0),), tag="extra-row-option"),
            Case("predict", 14, 2, 4, 300, m=5, tag="extra-row-K4"),
            Case("predict", 120, 3, 2, 40, m=5, tag="extra-row-n120"),
            Case("predict", 130, 3, 2, 4, m=3, tier="blocked"),
            Case("predict", 14, 1, 2, 2, m=3, tier="blocked", matern=True, tag="matern")]


def summary_cases():
    return [Case("summary", 14, 2, 2, 257, m=5, kept=True, tag="all-buffers"),
            Case("summary", 14, 2, 2, 257, m=5, kept=True, optional=False, tag="bare"),
            Case("summary", 130, 3, 2, 4, m=3, tier="blocked")]


def test_cases_sit_on_the_routes_they_name():
    """The shapes against tests/route_witnesses.py: the first blocked likelihood is n = 129, the first blocked Gaussian
    prediction of n <= 128 is far from every small case here (d = 63); the tier each case takes is asserted from the timing
    counters where it runs."""
    w = {(op, r): (n, d, K) for op, r, n, d, K in route_witnesses.WITNESSES[0]}
    assert w[("loglik", "b")][0] == 129 and w[("predict", "b")] == (108, 63, 1)
    for c in loglik_cases() + predict_cases() + summary_cases():
        assert (c.tier == "small") == (c.n <= 128 and not c.matern), c.id
        assert not c.kept or (c.n <= 104 and c.K <= 3 and c.tier == "small"), c.id


# ----------------------------------------------------------------------------- one case, end to end
def problem(torch, c):
    """numpy inputs of a case and their device images (column-major, flat)."""
    rng = np.random.default_rng(1000 * c.n + 10 * c.d + c.K)
    if c.matern:
        X = np.sort((np.arange(c.n) + rng.uniform(0.2, 0.8, c.n)) / c.n)[:, None]
        y = np.sin(9.0 * X[:, 0]) + 0.3 * np.cos(31.0 * X[:, 0])
        P = np.column_stack([rng.uniform(0.3, 0.9, c.B), rng.uniform(0.1, 0.7, c.B), rng.uniform(1.5, 3.0, c.B) / c.n,
                             rng.uniform(0.3, 0.8, c.B) / c.n])
    else:
        if (c.n, c.d) == (14, 2):
            X = load_maximin(14)
            y = np.sin(2 * np.pi * X[:, 0]) + 3.0 * X[:, 1] ** 2 + 5.0
        else:
            X, y = synthetic_design(c.n, c.d, seed=c.n + c.d)
        P = draws(rng, c.n, c.d, c.K, c.B)
    host = dict(X=X, y=y, P=P)
    if c.m:
        host["Xt"] = rng.random((c.m, c.d))
    if c.entry == "summary" and c.optional:
        host["y_at"] = np.linspace(float(y.min()), float(y.max()), c.m)
    dev = torch.device("cuda:0")
    true = {k: torch.tensor(np.asarray(v, dtype=np.float64).ravel(order="F"), device=dev) for k, v in host.items()}
    live = {k: torch.empty_like(v) for k, v in true.items()}
    return host, true, live


def output_tensors(torch, c):
    dev = torch.device("cuda:0")
    f = lambda k: torch.empty(k, dtype=torch.float64, device=dev)           # noqa: E731
    i = lambda k: torch.empty(k, dtype=torch.int32, device=dev)             # noqa: E731
    if c.entry == "loglik":
        outs = dict(loglik=f(c.B), beta=f(c.B), status=i(c.B))
    elif c.entry == "predict":
        outs = dict(mean=f(c.B * c.m), var=f(c.B * c.m), beta=f(c.B), status=i(c.B))
    else:
        outs = dict(out=f(c.m * (4 + len(LEVELS))))
        if c.optional:
            outs.update(beta=f(c.B), status=i(c.B))
    return outs, {k: torch.empty_like(v) for k, v in outs.items()}


SIGMA2, TAU2 = 1.3, 25.0


def dev_call(h, c, live, outs):
    if c.entry == "loglik":
        h.loglik_batch_dev(live["X"], c.n, c.d, live["y"], c.K, live["P"], c.B, SIGMA2, c.mode, TAU2 if c.mode else 0.0,
                           outs["loglik"], outs["beta"], outs["status"])
    elif c.entry == "predict":
        h.predict_batch_dev(live["X"], c.n, c.d, live["y"], c.K, live["P"], c.B, live["Xt"], c.m, SIGMA2, outs["mean"],
                            outs["var"], outs["beta"], outs["status"])
    else:
        h.predict_summary_dev(live["X"], c.n, c.d, live["y"], c.K, live["P"], c.B, live["Xt"], c.m, SIGMA2, LEVELS,
                              live.get("y_at"), outs["out"], outs.get("beta"), outs.get("status"))


def host_call(h, c, host):
    """The host-pointer entry point of the case, in the flat column-major form of the device buffers."""
    X, y, P = host["X"], host["y"], host["P"]
    if c.entry == "loglik":
        ll, beta, st = h.loglik_batch(X, y, c.K, P, SIGMA2, c.mode, TAU2 if c.mode else 0.0)
        return dict(loglik=ll, beta=beta, status=st)
    if c.entry == "predict":
        mean, var, beta, st = h.predict_batch(X, y, c.K, P, host["Xt"], SIGMA2)
        return dict(mean=mean.ravel(order="F"), var=var.ravel(order="F"), beta=beta, status=st)
    r = h.predict_summary(X, y, c.K, P, host["Xt"], SIGMA2, LEVELS, host.get("y_at"))
    out = np.column_stack([r["y_hat"], r["pred_var"], r["quant"], r["cdf_at"], r["quantiles"]])
    return dict(out=out.ravel(order="F"), beta=r["beta"], status=r["status"])


def new_handle(c):
    api = _api()
    h = api.Handle(0)
    for opt, val in c.options:
        h.set_option(opt, val)
    if c.limit is not None:
        h.set_workspace_limit(c.limit)
    if c.matern:
        h.set_kernel(api.KERNEL_MATERN, 2.5)
    return h


def assert_tier(c, t):
    if c.tier == "small":
        assert t["fused"][1] > 0 and t["diag"][1] == 0 and t["update"][1] == 0 and t["sweep"][1] == 0, t
    elif c.tier == "sched":
        assert t["sweep"][1] > 0 and t["fused"][1] == 0, t
    else:
        assert t["fused"][1] == 0 and t["sweep"][1] == 0 and t["diag"][1] > 0 and (c.n <= 128 or t["update"][1] > 0), t
        assert c.tier != "chunks" or t["solve"][1] >= 3, t


def assert_same_bits(c, got, want):
    for k, v in got.items():
        assert np.array_equal(_bits(v), _bits(want[k])), (c.id, k, v[:4], want[k][:4])


def warm_up(torch, c, stream, live, true, outs):
    """The same call once on the same stream through a throw-away handle (module docstring)."""
    w = new_handle(c)
    try:
        w.set_stream(stream.cuda_stream)
        for k in live:
            live[k].copy_(true[k])
        torch.cuda.synchronize()
        dev_call(w, c, live, outs)
        w.synchronize()
    finally:
        w.close()


def staged_on(torch, stream, delay, h, c, live, true, outs, snaps):
    """One staged call of case c through handle h (already on `stream`); asserts pending, returns the snapshots on the host."""
    pending = staged_call(torch, stream, delay, lambda: dev_call(h, c, live, outs),
                          [(live[k], true[k]) for k in live], [(outs[k], snaps[k]) for k in outs])
    assert pending, "%s: the call returned only after the %.0f ms of work enqueued before it" % (c.id, delay.ms)
    return {k: v.cpu().numpy() for k, v in snaps.items()}


def run_reserved(torch, stream, delay, c, check_free_memory=False):
    """Fresh handle on `stream`, reserve, one staged call: no figure of the handle changes, the delay is pending at return,
    the snapshots have the bits of the host-pointer call.  Returns (snapshots, reference, workspace figures)."""
    host, true, live = problem(torch, c)
    outs, snaps = output_tensors(torch, c)
    warm_up(torch, c, stream, live, true, outs)
    h = new_handle(c)
    try:
        h.set_stream(stream.cuda_stream)
        h.reserve(c.n, c.d, c.K, c.B, c.m)
        before = h.workspace_bytes()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        got = staged_on(torch, stream, delay, h, c, live, true, outs, snaps)
        free1 = torch.cuda.mem_get_info()[0]
        after = h.workspace_bytes()
        print("%s: workspace %d B, staging %d B; free memory %d -> %d" % ((c.id,) + before + (free0, free1)))
        assert after == before, (c.id, before, after)
        if c.tier == "small":
            assert before[0] == (kept_ws(c.n, c.m, c.B, c.limit) if c.kept else 0), (c.id, before)
        else:
            assert before[0] > 0, (c.id, before)
        if check_free_memory:
            assert before[0] >= 64 << 20 and free1 == free0, (c.id, before, free0, free1)
        want, t = _timed(h, lambda: host_call(h, c, host))
    finally:
        h.close()
    assert_tier(c, t)
    assert not want["status"].any(), (c.id, want["status"])
    assert_same_bits(c, got, want)
    return got, want, before


@pytest.mark.parametrize("c", loglik_cases(), ids=lambda c: c.id)
def test_loglik_dev_staged(torch, stream, delay, c):
    run_reserved(torch, stream, delay, c)


@pytest.mark.parametrize("c", predict_cases(), ids=lambda c: c.id)
def test_predict_dev_staged(torch, stream, delay, c):
    """The kept-factor cases fork the correlation vectors onto the handle's second stream and join them before the site
    solves; under the 1 MiB limit the 200 draws go in four chunks of 64 that fork and join again over the same scratch, and
    must equal the one-chunk result of an unlimited handle."""
    got, want, figures = run_reserved(torch, stream, delay, c)
    if c.limit is not None:
        assert figures[0] == 64 * sites_scratch(c.n, c.m) < c.B * sites_scratch(c.n, c.m)
        host = problem(torch, c)[0]
        whole = Case("predict", c.n, c.d, c.K, c.B, m=c.m, kept=True)
        h = new_handle(whole)
        try:
            one_chunk = host_call(h, whole, host)
            assert h.workspace_bytes()[0] == kept_ws(c.n, c.m, c.B)
        finally:
            h.close()
        assert_same_bits(c, got, one_chunk)


@pytest.mark.parametrize("c", summary_cases(), ids=lambda c: c.id)
def test_predict_summary_dev_staged(torch, stream, delay, c):
    got, want, _ = run_reserved(torch, stream, delay, c)
    if not c.optional:
        assert np.isnan(got["out"].reshape((c.m, -1), order="F")[:, 3]).all()


def test_reserved_kept_factor_scratch_of_64_mib_leaves_free_memory_alone(torch, stream, delay):
    """n = 100, S = 1000 (the reference's number of draws), m = 5: 95 424 B per draw, 91 MiB in all -- large enough that an
    allocation inside the call would show in the device's free memory, a witness that does not rest on
    ccgp_workspace_bytes."""
    c = Case("predict", 100, 3, 2, 1000, m=5, kept=True)
    assert sites_scratch(c.n, c.m) == 95424 and kept_ws(c.n, c.m, c.B) >= 64 << 20
    run_reserved(torch, stream, delay, c, check_free_memory=True)


def test_fewer_draws_than_reserved_need_nothing_more(torch, stream, delay):
    """reserve for S = 100; a call with S = 100 and then one with S = 50 leave the figures where reserve put them."""
    big, small = Case("predict", 14, 2, 2, 100, m=5, kept=True), Case("predict", 14, 2, 2, 50, m=5, kept=True)
    h = new_handle(big)
    try:
        h.set_stream(stream.cuda_stream)
        h.reserve(big.n, big.d, big.K, big.B, big.m)
        figures = h.workspace_bytes()
        assert figures[0] == kept_ws(14, 5, 100)
        for c in (big, small):
            host, true, live = problem(torch, c)
            outs, snaps = output_tensors(torch, c)
            torch.cuda.synchronize()
            got = staged_on(torch, stream, delay, h, c, live, true, outs, snaps)
            assert h.workspace_bytes() == figures, (c.id, figures, h.workspace_bytes())
            assert_same_bits(c, got, host_call(h, c, host))
    finally:
        h.close()


def test_stream_selection(torch, stream, delay):
    """A handle moved from stream A to stream B (synchronised in between) and then back to its own stream (set_stream(0):
    NOT torch's default stream, whatever pointer that reports) gives the same bits each time."""
    c = Case("predict", 14, 2, 2, 257, m=5, kept=True)
    host, true, live = problem(torch, c)
    outs, snaps = output_tensors(torch, c)
    other = torch.cuda.Stream()
    assert other.cuda_stream != stream.cuda_stream and other.cuda_stream != 0 and stream.cuda_stream != 0
    h = new_handle(c)
    try:
        h.reserve(c.n, c.d, c.K, c.B, c.m)
        figures = h.workspace_bytes()
        h.set_stream(stream.cuda_stream)
        torch.cuda.synchronize()
        on_a = staged_on(torch, stream, delay, h, c, live, true, outs, snaps)
        h.synchronize()
        h.set_stream(other.cuda_stream)
        on_b = staged_on(torch, other, delay, h, c, live, true, outs, snaps)
        h.synchronize()
        h.set_stream(0)
        for k in live:
            live[k].copy_(true[k])
        for v in outs.values():
            v.fill_(SENTINEL if v.dtype == torch.float64 else SENTINEL_INT)
        torch.cuda.synchronize()
        dev_call(h, c, live, outs)
        h.synchronize()
        on_own = {k: v.cpu().numpy() for k, v in outs.items()}
        assert h.workspace_bytes() == figures
        want = host_call(h, c, host)
    finally:
        h.close()
    for got in (on_a, on_b, on_own):
        assert_same_bits(c, got, want)
