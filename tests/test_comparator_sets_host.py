"""The comparator fits of a simulation study in lockstep across training sets (fit.ordinary_kriging_fit_sets, cgp.CGP_sets,
fit.study(lockstep_fits=...)) without a GPU.  The handle is a host stand-in (host_handles.SetsHandle): profile_batch and cgp_state_batch / cgp_predict
are the fp64 restatements tests/test_profile_ref.py and tests/test_cgp_ref.py already run the fits on, and its *_sets methods
call its own single-set methods set by set -- so what is held here is the host arithmetic around the device calls: a set's
fit in the group is its fit alone, bit for bit, and the group makes as many evaluator calls as its slowest set.  Every
comparison of outputs is np.testing.assert_array_equal on float64, no tolerance.

The stand-in remembers every evaluation by its operands' bytes, which changes no value and lets the second arm of a
comparison (the group after the per-set fits, the study with lockstep_fits on after off) cost next to nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import synthetic_design
from host_handles import SetsHandle
from ccgp_amd import api, cgp, design, fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ccgp_profile_batch_sets", "ccgp_cgp_state_batch_sets")


def _same_dict(got, want, skip=()):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in skip:
            continue
        if isinstance(want[k], np.ndarray):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        else:
            assert got[k] == want[k], k


@pytest.fixture(scope="module")
def three_sets():
    """3 sets of n = 12, d = 2: designs, responses with a trend that differs per set, six test points each."""
    sets = []
    for c in range(3):
        X, y = synthetic_design(12, 2, 40 + c)
        Xt, yt = synthetic_design(6, 2, 70 + c)
        sets.append((X, y * (1.0 + 0.2 * c) + 0.3 * c * X[:, 0], Xt, yt * (1.0 + 0.2 * c) + 0.3 * c * Xt[:, 0]))
    return sets


@pytest.fixture(scope="module")
def host(three_sets):
    """The stand-in handle with the per-set fits already made on it: ordinary_kriging_fit and CGP (two starts) per set."""
    h = SetsHandle()
    krige = [fit.ordinary_kriging_fit(h, s[0], s[1], starts=4, rng=c) for c, s in enumerate(three_sets)]
    cgps = [cgp.CGP(h, s[0], s[1], num_starts=2, rng=c + 5) for c, s in enumerate(three_sets)]
    return h, krige, cgps


# ----------------------------------------------------------------------------- minimize_starts: per-start bounds
def test_per_start_bounds_reproduce_separate_runs():
    """Two quadratic problems with different boxes (one optimum inside its box, one outside), three starts each."""
    rng = np.random.default_rng(3)
    centre = np.array([[0.3, -0.2, 0.1], [2.0, 0.5, -1.5]])
    lo, hi = np.array([[-1.0, -1.0, -1.0], [-0.5, 0.0, -1.0]]), np.array([[1.0, 1.0, 1.0], [1.5, 2.0, 0.25]])
    scale = np.array([1.0, 7.0, 0.4])
    starts = [lo[c] + rng.random((3, 3)) * (hi[c] - lo[c]) for c in range(2)]
    owner = np.repeat([0, 1], 3)

    def f_of(X, c):
        r = X - centre[c]
        return (scale * r ** 2).sum(axis=1) + 0.1 * (r ** 4).sum(axis=1), 2.0 * scale * r + 0.4 * r ** 3, np.zeros(len(X), dtype=int)

    log = []

    def together(X, live):
        log.append(list(live))
        parts = [f_of(X[i:i + 1], owner[s]) for i, s in enumerate(live)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))

    both = design.minimize_starts(together, np.concatenate(starts), lowers=lo[owner], uppers=hi[owner], pass_live=True)
    for c in range(2):
        alone = design.minimize_starts(lambda X, c=c: f_of(X, c), starts[c], lower=lo[c], upper=hi[c])
        sl = slice(3 * c, 3 * c + 3)
        for k in ("x", "f", "converged", "iterations"):
            np.testing.assert_array_equal(both[k][sl], alone[k])
        assert both["message"][sl] == alone["message"]
        assert both["calls_per_start"][sl].max() == alone["calls"]
        assert np.all((both["x"][sl] >= lo[c]) & (both["x"][sl] <= hi[c]))
    assert both["calls"] == both["calls_per_start"].max() == len(log) and all(l == sorted(l) for l in log)
    assert both["x"][3:, 0].max() == 1.5        # the second problem's optimum lies beyond its own upper bound, not the first's
    # the shared forms keep their meaning
    np.testing.assert_array_equal(design.minimize_starts(lambda X: f_of(X, 0), starts[0], lower=-1.0, upper=1.0)["x"], both["x"][:3])
    with pytest.raises(ValueError):
        design.minimize_starts(together, np.concatenate(starts), lowers=lo[owner], pass_live=True)
    with pytest.raises(ValueError):
        design.minimize_starts(together, np.concatenate(starts), lowers=lo, uppers=hi, pass_live=True)


# ----------------------------------------------------------------------------- the sigma2 / single-GP fit
def test_kriging_fits_in_lockstep_are_the_per_set_fits(three_sets, host):
    h, krige, _ = host
    before = dict(h.calls)
    got = fit.ordinary_kriging_fit_sets(h, [s[0] for s in three_sets], [s[1] for s in three_sets], starts=4, rng=[0, 1, 2])
    made = {k: h.calls[k] - before[k] for k in before}
    assert len(got) == 3
    for c in range(3):
        _same_dict(got[c], krige[c])
    counts = [k["calls"] for k in krige]
    print("per-set evaluator calls (final one included): %s; the group made %d" % (counts, made["profile_batch_sets"]))
    assert made["profile_batch_sets"] == max(counts) < sum(counts)       # the largest per-set count, not the sum
    assert made["profile_batch"] == 0 and len(set(counts)) > 1            # the sets do stop at different steps
    # one seed for every set is what C separate default fits take
    same_seed = fit.ordinary_kriging_fit_sets(h, [s[0] for s in three_sets[:2]], [s[1] for s in three_sets[:2]], starts=4)
    _same_dict(same_seed[0], krige[0])
    _same_dict(same_seed[1], fit.ordinary_kriging_fit(h, three_sets[1][0], three_sets[1][1], starts=4))


def test_kriging_fit_sets_checks_its_arguments(three_sets):
    h = SetsHandle()
    Ds, ys = [s[0] for s in three_sets], [s[1] for s in three_sets]
    for bad in (lambda: fit.ordinary_kriging_fit_sets(h, [], []),
                lambda: fit.ordinary_kriging_fit_sets(h, Ds, ys[:2]),
                lambda: fit.ordinary_kriging_fit_sets(h, [Ds[0], Ds[1][:11]], [ys[0], ys[1][:11]]),
                lambda: fit.ordinary_kriging_fit_sets(h, Ds, [ys[0], ys[1], ys[2][:11]]),
                lambda: fit.ordinary_kriging_fit_sets(h, Ds, ys, rng=[0, 1])):
        with pytest.raises(ValueError):
            bad()
    assert not any(h.calls.values())


# ----------------------------------------------------------------------------- CGP
OWN = ("calls", "evaluations", "refinement_calls", "seconds")


def test_cgp_fits_in_lockstep_are_the_per_set_fits(three_sets, host):
    h, _, cgps = host
    before = dict(h.calls)
    got = cgp.CGP_sets(h, [s[0] for s in three_sets], [s[1] for s in three_sets], num_starts=2, rngs=[5, 6, 7])
    made = {k: h.calls[k] - before[k] for k in before}
    for c in range(3):
        _same_dict(got[c], cgps[c], skip=OWN)
        assert got[c]["evaluations"] == cgps[c]["evaluations"]            # a set's rows are the rows it has alone
    ref_calls = [e["refinement_calls"] for e in cgps]
    print("per-set refinement calls %s; the group made %d" % (ref_calls, got[0]["refinement_calls"]))
    assert got[0]["refinement_calls"] == max(ref_calls) < sum(ref_calls)
    # candidates and jackknife are one call each, the final states one per set
    assert made == dict(profile_batch=0, profile_batch_sets=0, cgp_state_batch=0, cgp_state_batch_sets=max(ref_calls) + 2,
                        cgp_predict=3)
    assert all(e["calls"] == max(ref_calls) + 2 + 3 for e in got)


def test_cgp_sets_checks_its_arguments(three_sets):
    h = SetsHandle()
    Ds, ys = [s[0] for s in three_sets], [s[1] for s in three_sets]
    for bad in (lambda: cgp.CGP_sets(h, [], []),
                lambda: cgp.CGP_sets(h, Ds, ys[:2]),
                lambda: cgp.CGP_sets(h, [Ds[0], Ds[1][:, :1]], ys[:2]),
                lambda: cgp.CGP_sets(h, Ds, ys, rngs=[1, 2]),
                lambda: cgp.CGP_sets(h, Ds, ys, theta_l=1e9)):
        with pytest.raises(ValueError):
            bad()
    assert not any(h.calls.values())


# ----------------------------------------------------------------------------- compare_GP and the study
class HostGP:
    """What compare_GP and study ask of a CombinedGP, on the stand-in handle."""
    script = "GV"
    cfg = dict(prior=api.PRIOR_GV, npar=3)

    def __init__(self, h):
        self.h = h

    def prediction(self, D_test, alpha, draws, D_train, sigma2, y_train):
        m = len(D_test)
        centre = np.full(m, float(np.mean(y_train))) + float(np.mean(draws)) * np.asarray(D_test)[:, 0]
        half = np.sqrt(sigma2) * np.ones(m)
        return dict(y_hat=centre, Quant=np.full(m, 0.5), LL=centre - half, UL=centre + half)


def test_compare_gp_takes_fitted_models_and_fits_nothing(three_sets, host):
    h, krige, cgps = host
    D, y, Dt, yt = three_sets[0]
    gp = HostGP(h)
    draws = np.array([[0.5, 1.0, 9.0]])
    fitted = fit.compare_GP(gp, Dt, 0.05, yt, draws, D, 1.0, y, exact=True, cgp=dict(num_starts=2, rng=5),
                            single=dict(starts=4, rng=0))
    before = dict(h.calls)
    given = fit.compare_GP(gp, Dt, 0.05, yt, draws, D, 1.0, y, exact=True, cgp=dict(est=cgps[0]), single=dict(est=krige[0]))
    made = {k: h.calls[k] - before[k] for k in before}
    assert made == dict(profile_batch=0, profile_batch_sets=0, cgp_state_batch=0, cgp_state_batch_sets=0, cgp_predict=1)
    assert given["CGP"] is cgps[0] and given["single"] is krige[0]
    for k in ("y_hat", "LL", "UL", "y_hat_CGP", "LL_CGP", "UL_CGP", "y_hat_single", "LL_single", "UL_single"):
        np.testing.assert_array_equal(given[k], fitted[k], err_msg=k)
    _same_dict(fitted["single"], krige[0])
    _same_dict(fitted["CGP"], cgps[0], skip=("seconds",))


def test_study_gives_the_same_tables_with_lockstep_fits_on_and_off(three_sets, host):
    h = host[0]
    gp = HostGP(h)
    arms = {}
    for on in (False, True):
        before = dict(h.calls)
        arms[on] = fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], cgp=dict(num_starts=2),
                             single=True, lockstep_fits=on)
        arms[on]["made"] = {k: h.calls[k] - before[k] for k in before}
    off, on = arms[False], arms[True]
    assert off["made"]["profile_batch_sets"] == 0 and off["made"]["cgp_state_batch_sets"] == 0
    assert on["made"]["profile_batch"] == 0 and on["made"]["cgp_state_batch"] == 0
    assert on["sigma2"] == off["sigma2"]
    for i in range(3):
        assert sorted(on["tables"][i]) == sorted(off["tables"][i])
        for k, v in off["tables"][i].items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(on["tables"][i][k], v, err_msg=k)
        _same_dict(on["tables"][i]["single"], off["tables"][i]["single"])
        _same_dict(on["tables"][i]["CGP"], off["tables"][i]["CGP"], skip=OWN)
        assert on["summaries"][i] == off["summaries"][i]
        np.testing.assert_array_equal(on["draws"][i], off["draws"][i])
        np.testing.assert_array_equal(on["chains"][i]["sample"], off["chains"][i]["sample"])
    assert on["pooled"] == off["pooled"]
    # the single GP is fitted a second time per set only without the lockstep fits; with them sigma2's model is handed over
    assert off["calls"]["single"] == off["calls"]["sigma2"] > 0 and on["calls"]["single"] == 0
    assert 0 < on["calls"]["sigma2"] < off["calls"]["sigma2"] and 0 < on["calls"]["cgp"] < off["calls"]["cgp"]
    for k in ("laplace", "metro", "predict"):
        assert on["calls"][k] == off["calls"][k]
    assert set(on["seconds"]) == set(on["calls"]) == {"sigma2", "single", "cgp", "laplace", "metro", "predict"}
    # where the device is replaced the per-set loop stays: compare_fn sees the arguments as given
    seen = []

    def compare(gp, D_test, alpha, y_test, draws, D_train, sigma2, y_train, exact, cgp, single):
        seen.append((cgp, single))
        return off["tables"][len(seen) - 1]
    before = dict(h.calls)
    fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], sigma2s=off["sigma2"], cgp=True,
              single=True, compare_fn=compare)
    assert seen == [(True, True)] * 3 and h.calls == before


def _same_tables(on, off):
    for i in range(len(off["tables"])):
        assert sorted(on["tables"][i]) == sorted(off["tables"][i])
        for k, v in off["tables"][i].items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(on["tables"][i][k], v, err_msg=k)
        _same_dict(on["tables"][i]["single"], off["tables"][i]["single"])
        _same_dict(on["tables"][i]["CGP"], off["tables"][i]["CGP"], skip=OWN)
        assert on["summaries"][i] == off["summaries"][i]


def test_study_passes_a_cgp_seed_on_to_every_set(three_sets, host):
    """cgp=dict(rng=seed) is cgp.CGP's keyword: per set a fresh default_rng(seed), in lockstep CGP_sets' rngs=[seed] * C."""
    h = host[0]
    gp = HostGP(h)
    arms = {}
    for on in (False, True):
        before = dict(h.calls)
        arms[on] = fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3],
                             cgp=dict(num_starts=2, rng=5), single=True, lockstep_fits=on)
        arms[on]["made"] = {k: h.calls[k] - before[k] for k in before}
    _same_tables(arms[True], arms[False])
    assert arms[True]["made"]["cgp_state_batch"] == 0 and arms[True]["made"]["cgp_state_batch_sets"] > 0
    assert 0 < arms[True]["calls"]["cgp"] < arms[False]["calls"]["cgp"]
    # the seed is used: set 0's model is the fixture's CGP(..., rng=5), not the default seed's
    _same_dict(arms[True]["tables"][0]["CGP"], host[2][0], skip=OWN)
    default = cgp.CGP(h, three_sets[0][0], three_sets[0][1], num_starts=2)
    assert not np.array_equal(default["starts"], host[2][0]["starts"])


def test_study_keeps_one_cgp_generator_advancing_from_set_to_set(three_sets, host):
    """A Generator in cgp's dict is one stream that every set's CGP draws from in turn: those fits stay per set."""
    h = host[0]
    gp = HostGP(h)
    arms = {}
    for on in (False, True):
        before = dict(h.calls)
        arms[on] = fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3],
                             cgp=dict(num_starts=2, rng=np.random.default_rng(5)), single=True, lockstep_fits=on)
        arms[on]["made"] = {k: h.calls[k] - before[k] for k in before}
    _same_tables(arms[True], arms[False])
    assert arms[True]["made"]["cgp_state_batch_sets"] == 0            # the CGP fits went set by set
    assert arms[True]["made"]["profile_batch"] == 0                   # sigma2 and the single GP still in lockstep
    assert arms[True]["calls"]["cgp"] == arms[False]["calls"]["cgp"] > 0


def test_study_charges_time_where_it_counts_calls(three_sets, host):
    """Every sigma2 given and single=True: the shared fit is the single GP's alone, in calls and in seconds."""
    gp = HostGP(host[0])
    s2 = [float(f["sigma2"]) for f in host[1]]
    r = fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], sigma2s=s2, single=True)
    assert r["calls"]["sigma2"] == 0 and r["seconds"]["sigma2"] == 0.0
    assert r["calls"]["single"] > 0 and r["seconds"]["single"] > 0.0
    r = fit.study(gp, three_sets, 0.05, 120, 40, 10, 0.5, net_samp_size=30, rngs=[1, 2, 3], single=True)
    assert r["calls"]["sigma2"] > 0 and r["seconds"]["sigma2"] > 0.0 and r["calls"]["single"] == 0


# ----------------------------------------------------------------------------- the Python wrappers' own checks, the symbols
def test_wrappers_refuse_before_they_call_the_library(monkeypatch):
    monkeypatch.setattr(api, "lib", lambda: pytest.fail("the library was called"))
    h = api.Handle.__new__(api.Handle)
    Xs, ys = np.zeros((2, 5, 2)), np.zeros((2, 5))
    set_of = np.array([0, 1, 1])
    for bad in (lambda: h.profile_batch_sets(Xs[0], ys, 1, np.ones((3, 3)), set_of),            # one design, not [C, n, d]
                lambda: h.profile_batch_sets(Xs, ys, 1, np.ones((3, 4)), set_of),               # K + K d = 3 columns
                lambda: h.profile_batch_sets(Xs, ys, 1, np.ones((3, 3)), set_of[:2]),           # one set index per row
                lambda: h.profile_batch_sets(Xs, ys[:, :4], 1, np.ones((3, 3)), set_of),        # ys is [C, n]
                lambda: h.profile_batch_sets(1.0, ys, 1, np.ones((3, 3)), set_of),              # no design at all
                lambda: h.cgp_state_batch_sets(1.0, ys, np.ones((3, 6)), set_of),
                lambda: h.cgp_state_batch_sets(Xs[0], ys, np.ones((3, 6)), set_of),
                lambda: h.cgp_state_batch_sets(Xs, ys, np.ones((3, 5)), set_of),                # 2 d + 2 = 6 columns
                lambda: h.cgp_state_batch_sets(Xs, ys, np.ones((3, 6)), set_of[:2]),
                lambda: h.cgp_state_batch_sets(Xs, ys, np.ones((3, 6)), set_of, skip=[0, 1])):  # one skip per row
        with pytest.raises(ValueError):
            bad()


def test_new_symbols_are_in_the_header_the_bindings_and_the_library():
    header = open(os.path.join(ROOT, "include", "ccgp.h")).read()
    for name in NEW:
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
        assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == n_args, name
    from ccgp_amd import library_path
    assert os.path.exists(library_path()), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = ctypes.CDLL(library_path())
    for name in NEW:
        assert hasattr(L, name), name
