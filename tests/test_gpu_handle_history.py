"""A call's bits must not depend on what its handle ran before.

The handle's buffers only grow (csrc/capi.hip: ensure), blocked_carve lays the same bytes out differently for every
(npad, nb, ne), and the workspace is memset in a handful of places only: elsewhere the library rests on "this word is
written before it is read, in the same call".  A fresh hipMalloc usually hands out zero pages, so a read of a
never-written word returns 0.0 or status 0 and nothing else in the suite notices.  Here every subject of
tests/history_cases.py (every batched entry point, every route, every variant of the sweep) runs

  a. after Handle.debug_fill_scratch(0x00), (0x3F) and (0xFF): workspace, staging and pinned buffer hold zeros, then
     finite doubles near 4.7e-4 with the int 1061109567, then NaNs with the int -1 -- and every buffer the call itself
     allocates starts with the same bytes;
  b. on a handle too small for it, so that the subject itself regrows the buffer under the fill on allocation;
  c. inside a seeded sequence of about 40 other subjects on one handle, with the handle's options, kernel family,
     workspace limit and stream changed and restored in between, and no hook at all;

and must return, every time, the bits it returns on a handle created for it alone: every value, every optional output,
status and the C return values.  Doubles are compared as uint64 (a NaN's payload counts), integers with
assert_array_equal.  There is no tolerance in this file, no skip and no list of known differences.

The reference of a subject is computed once (on a fresh handle that was never filled) and shared by all three parts.
Handles of this module are created under CCGP_SCHED_TIMEOUT_MS = 3000: a stale control word of the scheduler then costs
seconds and a failed chunk, not the default 30 s.
"""
import os

import numpy as np
import pytest

import history_cases as hc
import test_gpu_routes

pytestmark = pytest.mark.gpu
TABLE = hc.table()
FILLS = (0x00, 0x3F, 0xFF)
_REF = {}


class fresh:
    """A handle (or ccgp_multi) of the subject's kind, created under the short scheduler timeout, closed on exit."""

    def __init__(self, subject=None):
        self.subject = subject

    def __enter__(self):
        old = os.environ.get("CCGP_SCHED_TIMEOUT_MS")
        os.environ["CCGP_SCHED_TIMEOUT_MS"] = "3000"
        try:
            self.h = self.subject.factory() if self.subject else hc.new_handle()
        finally:
            if old is None:
                del os.environ["CCGP_SCHED_TIMEOUT_MS"]
            else:
                os.environ["CCGP_SCHED_TIMEOUT_MS"] = old
        return self.h

    def __exit__(self, *exc):
        self.h.close()


def reference(s):
    """The subject on a handle created for it alone, never filled; checked once: passing rows finite with status 0, the
    singular row NaN with its derived pivot."""
    if s.id not in _REF:
        with fresh(s) as h:
            out, _ = s.call(h)
        s.check(out)
        _REF[s.id] = out
    return _REF[s.id]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_bits(s, got, want, where):
    assert sorted(got) == sorted(want), (s.id, where)
    for k in want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (s.id, where, k)
        if w.dtype == np.float64:
            diff = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
            assert diff.size == 0, "%s %s: %s differs in %d of %d words, first at %d: %r, alone %r" % (
                s.id, where, k, diff.size, w.size, diff[0], g.ravel()[diff[0]], w.ravel()[diff[0]])
        else:
            np.testing.assert_array_equal(g, w, err_msg="%s %s: %s" % (s.id, where, k))


# ----------------------------------------------------------------------------- the table itself
def test_every_cell_has_its_subject():
    """Every (op, route) cell of tests/route_witnesses.py, as tests/test_gpu_routes.py lists them, at its witness shape."""
    cells = {s.cell: s for s in TABLE if s.cell}
    assert sorted(cells) == sorted(test_gpu_routes.CELLS)
    for cell, s in cells.items():
        n = test_gpu_routes.CELLS[cell][0]
        assert s.n == n and s.tier == {"r": "small", "l": "small", "b": "blocked", "u": None}[cell[1]], s.id


def test_every_entry_point_and_variant_has_its_subject():
    assert {s.entry for s in TABLE} == set(hc.ENTRY_POINTS)
    ids = {s.id for s in TABLE}
    for n in (257, 129):
        for tag in ("sched0", "sched1", "sched2", "fused-solve0", "fused-solve2", "fuse-diag0", "fuse-diag1", "tail-strips0",
                    "tail-strips1", "wide-offsets1"):
            assert "sweep-n%d-%s" % (n, tag) in ids
    assert sorted(s.id for s in TABLE if s.singular) == ["grad-blocked-n257+singular", "loglik-blocked-n129+singular",
                                                        "predict-kept-n64+singular", "summary-staged-n64+singular"]
    assert all(len(s.failing) == 1 for s in TABLE if s.failing)
    assert sum(s.multi for s in TABLE) == 2 and len({s.entry for s in TABLE if s.torch}) == 3


def test_one_case_per_subject():
    assert len(FILL_CASES) == len(TABLE) == len({s.id for s in TABLE})


# ----------------------------------------------------------------------------- a. fill patterns
FILL_CASES = [pytest.param(s, id=s.id) for s in TABLE]


@pytest.mark.parametrize("s", FILL_CASES)
def test_fill_patterns(s):
    want = reference(s)
    with fresh(s) as h:
        got, _ = s.call(h)                       # the handle now holds what the subject needs: the fills below have a target
        assert_same_bits(s, got, want, "on a second fresh handle")
        for byte in FILLS:
            got, before = s.call(h, fill=byte)   # Subject.call asserts that the fill returned 0
            assert not s.uses_ws or before[0] > 0, (s.id, before)
            assert before[0] + before[1] > 0 or "code" in want, (s.id, before)     # a refused call holds no buffer at all
            assert_same_bits(s, got, want, "after a fill with 0x%02X" % byte)


# ----------------------------------------------------------------------------- b. growth under the fill on allocation
# (subject, the figures of workspace_bytes() that must grow: 0 = workspace, 1 = staging): the sweep's workspace, the staging
# buffer alone, a factor set (allocated by the call, with the scratch rows of its prediction in the workspace), the
# kept-factor scratch
GROWTH = [("sweep-n257-sched0", (0, 1)), ("predict-blocked-n129-m129", (0, 1)), ("corr-n100-m70", (1,)), ("factorset-n257", (0,)),
          ("factorset-n257-m129", (0, 1)), ("predict-kept-n100-S66", (0, 1))]


@pytest.mark.parametrize("byte", [0x3F, 0xFF])
@pytest.mark.parametrize("sid,grows", GROWTH)
def test_regrown_buffers_start_filled(sid, grows, byte):
    """A handle that has only served a tiny call (a few KB of staging, no workspace) is filled, which also turns the fill
    on allocation on; the subject then regrows the buffers itself -- and, for the factor set, allocates the set -- and
    every new byte is `byte`."""
    s = next(x for x in TABLE if x.id == sid)
    tiny = next(x for x in TABLE if x.id == "loglik-n5-mode0")
    want = reference(s)
    with fresh(s) as h:
        got, _ = tiny.call(h)
        assert_same_bits(tiny, got, reference(tiny), "before the growth")
        small = h.workspace_bytes()
        assert small[0] == 0 and 0 < small[1] < 1 << 16, small
        got, before = s.call(h, fill=byte)
        grown = h.workspace_bytes()
        assert before == small and all(grown[k] > small[k] for k in grows), (sid, small, grown)
        assert_same_bits(s, got, want, "grown under a fill with 0x%02X" % byte)
        assert h.debug_fill_scratch(-1) == 0
        got, _ = s.call(h)
        assert_same_bits(s, got, want, "after the growth")


def test_fill_arguments():
    with fresh() as h:
        assert h.debug_fill_scratch(0) == 0 and h.debug_fill_scratch(255) == 0 and h.debug_fill_scratch(-1) == 0
        for bad in (-2, 256, 1 << 20):
            with pytest.raises(hc._api().CcgpError) as e:
                h.debug_fill_scratch(bad)
            assert e.value.code == -1
    assert hc._api().lib().ccgp_debug_fill_scratch(None, 0) == -1


def test_fill_forgets_the_scheduler_time_account():
    """The account of ccgp_last_sched_profile lies in the workspace the fill overwrites: after a fill there is none, rather
    than a thousand rows of 0x3F3F3F3F3F3F3F3F ticks."""
    s = next(x for x in TABLE if x.id == "sweep-n257-sched1")
    with fresh(s) as h:
        h.set_option(hc.SCHED_POLICY, 11 | 4)
        s.call(h)
        acc = h.last_sched_profile()
        assert acc.shape[0] > 0 and acc[:, 5].sum() > 0
        assert h.debug_fill_scratch(0x3F) == 0
        assert h.last_sched_profile().shape[0] == 0
        s.call(h)
        again = h.last_sched_profile()
        assert again.shape == acc.shape and again[:, 5].sum() == acc[:, 5].sum()      # the same number of tasks ran


# ----------------------------------------------------------------------------- c. natural histories
# (before, after): a larger call before a smaller one of the same entry point, a call whose every row fails before one
# whose every row passes, a scheduled sweep before a launch-per-phase sweep of another number of tiles and the reverse
PAIRS = [("sweep-n257-sched0", "cell-loglik-b"), ("predict-blocked-n129-m129", "predict-blocked-n129-m3"),
         ("grad-n257", "cell-grad-b"), ("predict-kept-n100-S66", "predict-kept-n64"), ("factorset-n257-m129", "factorset-n90"),
         ("all-fail-blocked-n129", "loglik-n129-mode1"), ("all-fail-kept-n64", "predict-kept-n64"),
         ("sweep-n257-sched1", "sweep-n129-sched0"), ("sweep-n257-sched0", "sweep-n129-sched1"),
         ("sweep-n129-sched2", "sweep-n257-fused-solve2"), ("summary-streamed-n14-S2049", "summary-staged-n64")]


def history(seed, length=40):
    """[(subject, modifier)]: the pairs above at random places among subjects drawn from the table."""
    rng = np.random.default_rng(seed)
    by_id = {s.id: s for s in TABLE}
    by_id.update(hc.interludes())
    pool = [s for s in TABLE if not s.multi]
    pairs = [PAIRS[i] for i in rng.permutation(len(PAIRS))[:7]]
    seq = []
    for k in range(length - 2 * len(pairs)):
        seq.append([pool[int(rng.integers(len(pool)))]])
    for a, b in pairs:
        seq.insert(int(rng.integers(len(seq) + 1)), [by_id[a], by_id[b]])
    out = []
    for group in seq:
        for s in group:
            mods = ["none", "options", "kernels", "stream", "none"] + ([] if s.torch or s.limit else ["limit"])
            out.append((s, mods[int(rng.integers(len(mods)))]))
    return out


def toggle_options(h, rng):
    """Set every option to another legal value and back: nothing may latch."""
    for opt, default in hc.OPTION_DEFAULTS.items():
        h.set_option(opt, {hc.SCHED: 1, hc.SCHED_POLICY: 9, hc.FUSED_SOLVE: 2}.get(opt, 1 - default))
    for opt in rng.permutation(list(hc.OPTION_DEFAULTS)):
        h.set_option(int(opt), hc.OPTION_DEFAULTS[int(opt)])


@pytest.mark.parametrize("seed", [20260501, 20260502])
def test_natural_history(seed):
    import torch
    rng = np.random.default_rng(seed + 1)
    stream = torch.cuda.Stream()
    seq = history(seed)
    assert 35 <= len(seq) <= 45
    done = []
    with fresh() as h:
        for s, mod in seq:
            want = reference(s)
            done.append("%s [%s]" % (s.id, mod))
            where = "as call %d of\n  %s" % (len(done), "\n  ".join(done))
            limit = None
            if mod == "options":
                toggle_options(h, rng)
            elif mod == "kernels":
                for fam in (hc.MATERN, hc.SPLINE, hc.GAUSS):
                    h.set_kernel(fam, 2.5 if fam else 0.0)
            elif mod == "limit":
                limit = 1 << 20          # the smallest limit there is: a sweep goes one matrix at a time
            elif mod == "stream":
                h.set_stream(stream.cuda_stream)
            try:
                got, _ = s.call(h, limit=limit)
            except AssertionError as e:
                raise AssertionError("%s\n%s" % (e, where))
            finally:
                if mod == "stream":
                    h.synchronize()
                    h.set_stream(0)
            assert_same_bits(s, got, want, where)


def test_histories_contain_what_they_are_for():
    for seed in (20260501, 20260502):
        seq = history(seed)
        ids = [s.id for s, _ in seq]
        assert sum(1 for a, b in PAIRS if any(ids[k:k + 2] == [a, b] for k in range(len(ids)))) >= 7
        assert {m for _, m in seq} >= {"options", "kernels", "stream", "limit"}
        assert len({s.id for s, _ in seq}) >= 25
