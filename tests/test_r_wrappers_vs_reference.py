"""r/ccgp.R cannot run in this container (no R).  Its wrappers around the scripts' own compare.GP / prediction / factors.frame
assume things about those scripts; this test checks every assumption against tests/golden/r_script_facts.json, the record
of those facts read off the eight reference scripts by tests/golden/make_r_script_facts.py (argument lists, column names,
counts and pattern checks -- no script text):
  * every `a$name` the compare.GP / prediction wrappers read is a formal argument of that script's own definition
    (the wrappers bind arguments with match.call against those formals);
  * each script's `prediction` body contains exactly ONE `apply(pars.frame, 1, predict.post` -- the call the wrapper answers
    from the batched table by swapping `apply` in the function's environment;
  * the leading columns factors.frame builds are (p, theta1, theta2[, lambda]), then beta: what .ccgp.layout / the shim's
    LAYOUT_* and `pars[o + 1] is beta` rely on (HX:631-643, ANI:572-592, D1:750-781);
  * logpost / factors / predict.post / Mixed.corr.* signatures match the definitions r/ccgp.R overrides them with."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "r_script_facts.json")) as _fh:
    FACTS = json.load(_fh)
SCRIPTS = sorted(FACTS)


def test_the_record_covers_the_eight_scripts():
    assert SCRIPTS == ["ADV", "ANI", "BSQ", "D1", "D1F", "GV", "HX", "ISO"]


def definition(src, name):
    """(formals, body) of the LAST top-level `name <- function(...) {...}` in an R source text."""
    hits = list(re.finditer(r"^%s\s*<-\s*function\s*\(" % re.escape(name), src, flags=re.M))
    if not hits:
        return None
    pos = hits[-1].end()
    depth, i = 1, pos
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    formals = [a.strip().split("=")[0].strip() for a in src[pos:i - 1].replace("\n", " ").split(",")]
    j = src.index("{", i)
    depth, k = 1, j + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        k += 1
    return formals, src[j:k]


def wrapper_reads(rsrc, name):
    """names read as a$<name> inside r/ccgp.R's wrapper `name <- function(...) {`"""
    _, body = definition(rsrc, name)
    return set(re.findall(r"\ba\$([A-Za-z.][A-Za-z0-9._]*)", body))


@pytest.fixture(scope="module")
def rsrc():
    with open(os.path.join(ROOT, "r", "ccgp.R")) as fh:
        src = fh.read()
    # the wrappers live inside `if (exists(...)) { ... }` blocks: dedent them so that `definition` sees top-level assignments
    return re.sub(r"^  (compare\.GP|prediction|factors\.frame) <- function", r"\1 <- function", src, flags=re.M)


@pytest.mark.parametrize("tag", SCRIPTS)
def test_wrapped_arguments_are_formals_of_the_script(rsrc, tag):
    for fn, alternatives in (("compare.GP", {"D.test": "D.new", "D.new": "D.test"}), ("prediction", {})):
        d = FACTS[tag]["formals"][fn]
        assert d is not None, "%s has no %s" % (tag, fn)
        formals = set(d)
        for name in wrapper_reads(rsrc, fn):
            if name == "nu":                 # read through .ccgp.nu(a): NULL where the script has no nu
                continue
            ok = name in formals or alternatives.get(name) in formals
            assert ok, "%s: the %s wrapper reads a$%s, formals are %s" % (tag, fn, name, sorted(formals))
        if tag in ("D1", "D1F"):
            assert "nu" in formals
        else:
            assert "nu" not in formals


@pytest.mark.parametrize("tag", SCRIPTS)
def test_prediction_has_exactly_one_apply_over_the_frame(tag):
    formals, facts = FACTS[tag]["formals"]["prediction"], FACTS[tag]["prediction"]
    calls = facts["apply_over_frame_calls"]
    assert calls == 1, "%s: %d apply(pars.frame, 1, predict.post ...) calls" % (tag, calls)
    assert facts["apply_calls"] == 1          # the wrapper swaps EVERY apply in that environment
    assert "pars.frame" in formals and "x.new" in formals and "D.train" in formals and "sigma2" in formals
    # what comes back is transposed into an S x 2 frame named mean / var: the 2 x S block the wrapper returns fits
    assert facts["returns_transposed_mean_var_frame"]


@pytest.mark.parametrize("tag", SCRIPTS)
def test_frame_columns_are_the_layout_the_shim_indexes(rsrc, tag):
    formals, facts = FACTS[tag]["formals"]["factors.frame"], FACTS[tag]["factors.frame"]
    cols = facts["samp_columns"]
    want = ["p", "theta1", "theta2", "lambda"] if tag == "ANI" else ["p", "theta1", "theta2"]
    assert cols == want, (tag, cols)
    assert facts["returns_samp_beta_factors_rinv"]
    # r/ccgp.R: layout 2 (four leading columns, anisotropic rates) for ANI only; ADV's frame is (p, theta1, theta2) like HX's
    lay = re.search(r"\.ccgp\.layout\s*<-\s*switch\(ccgp\.script,\s*([^)]*)\)", rsrc).group(1)
    table = dict((k.strip(), v.strip()) for k, v in (e.split("=") for e in lay.split(",") if "=" in e))
    default = [e.strip() for e in lay.split(",") if "=" not in e][0]
    got = table.get(tag, default)
    assert got == {"ANI": "2L", "D1": "3L", "D1F": "4L"}.get(tag, "0L"), (tag, got)
    # y.train and D.train are formals factors.frame hands on to factors(): the wrapper's attribute comes from there
    assert "y.train" in formals and "D.train" in formals
    assert facts["passes_n_train_y_train_to_factors"]


def test_where_each_predict_post_finds_beta_and_its_second_scale():
    """The shim's `pars[o + 1] is beta` with o = 4 for the anisotropic layout and 3 otherwise, and ADV's predict.post as written:
    third leading column used as lambda in theta1 * (1 + lambda) (ADV:672) although the frame stores theta2 there (ADV:639-641)
    -- the inconsistency LAYOUT_ADV_WRITTEN reproduces on request and the batched path resolves towards the training kernel."""
    shim = open(os.path.join(ROOT, "r", "ccgp_shim.c")).read()
    assert re.search(r"layout == LAYOUT_ANI \? 4 : 3;\s*/\* pars\[o \+ 1\] is beta", shim)
    for tag in SCRIPTS:
        col = 5 if tag == "ANI" else 4
        assert FACTS[tag]["predict.post"]["beta_column"] == col, (tag, col)
    adv = FACTS["ADV"]["predict.post"]
    assert adv["lambda_column"] == 3 and adv["scales_theta1_by_one_plus_lambda"]
    assert re.search(r"layout == LAYOUT_ADV_WRITTEN \? t1 \* \(1\.0 \+ t2\) : t2", shim)


@pytest.mark.parametrize("tag", SCRIPTS)
def test_overridden_signatures_match(tag):
    """The argument lists r/ccgp.R defines for this script's variant against the script's own."""
    want = {
        "logpost": {"HX": 6, "ADV": 6, "D1": 5, "D1F": 5}.get(tag, 4),
        "factors": 3,
        "predict.post": 5 if tag in ("D1", "D1F") else 4,
    }
    for fn, nargs in want.items():
        d = FACTS[tag]["formals"][fn]
        assert d is not None, (tag, fn)
        assert len(d) == nargs, (tag, fn, d)
    f = FACTS[tag]["formals"]["factors"]
    assert f == ["MCMC.data", "n.train", "y.train"]
    f = FACTS[tag]["formals"]["predict.post"]
    assert f[:4] == ["x.new", "D.train", "pars", "sigma2"]


@pytest.mark.parametrize("tag", ["HX", "GV", "ISO", "ADV", "ANI", "BSQ"])
def test_metro_loop_is_what_the_block_wise_metro_assumes(rsrc, tag):
    """r/ccgp.R's Metro pre-draws m iterations' random numbers.  That is the script's chain only if the script's loop draws
    exactly  u <- runif(1)  and then  rmnorm(1, as.vector(theta.old), sqrt(2)*pars$v)  per iteration, in this order, accepts on
    R > log(u) with R = l.cand$val - l.old$val, and runs Geweke's test on the first column of the last samp.size accepted draws
    whenever (k-1) >= samp.size & (k-1) %% batch.size == 0 -- and if every call site passes Metro's arguments by position."""
    formals, facts = FACTS[tag]["formals"]["Metro"], FACTS[tag]["Metro"]
    assert formals[:8] == ["start", "N", "samp.size", "batch.size", "alpha", "D.train", "sigma2", "y"]
    assert len(formals) == (10 if tag in ("HX", "ADV") else 9), formals
    assert facts["draws_runif_then_rmnorm_only"]
    assert facts["accepts_on_log_ratio"]
    assert facts["loops_while_k_le_N_and_pv_lt_alpha"]
    assert facts["geweke_every_batch_after_samp_size"]
    assert facts["geweke_on_last_samp_size_draws"]
    assert facts["starts_from_laplace_mode"]
    assert facts["returns_last_samp_size_with_rinv"]        # the list r/ccgp.R's Metro returns (it always adds BSQ's `logpost`)
    assert "logpost = log.posterior[(k - samp.size):(k - 1)]" in open(os.path.join(ROOT, "r", "ccgp.R")).read()
    # every call of Metro in the script passes its arguments by position
    assert facts["every_call_passes_arguments_by_position"]
    # r/ccgp.R's replacement takes the same number of arguments
    r_formals = re.search(r"Metro <- function\(([^)]*)\)\s*\n\s*\.ccgp\.Metro\(start, N, samp\.size, batch\.size, alpha, D\.train, sigma2, y,\s*\n\s*c\(\.ccgp\.prior",
                          open(os.path.join(ROOT, "r", "ccgp.R")).read())
    assert r_formals and len(r_formals.group(1).split(",")) == 10
