"""The CGP refinement's objective in portable arithmetic (csrc/cgp_fit_logic.h) against numpy, without a GPU.  The step kernel
of ccgp_cgp_fit_sets and its host twin form a start's parameter rows and its gradient with these functions, so they have to BE
cgp._fit_sets.evaluate and cgp.rows_from_ww: tests/host_small/cgp_fit_logic_check.cpp prints what the header makes of seeded
points -- interior ones, points on either bound and half a step from it (the clipped differences), values that are NaN or
infinite (the 1e6 of GV:130-131) -- and every row entry, f and gradient entry must have numpy's bits.  Built plain, and once as
a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ccgp_amd import cgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_small", "cgp_fit_logic_check.cpp")
CSRC = os.path.join(ROOT, "convex-combination-of-gaussian-processes_amd", "csrc")
DIMS = [1, 2, 3, 4, 9, 21, 61]


def _cases():
    rng = np.random.default_rng(20261020)
    out = []
    for d in DIMS:
        P = d + 3
        for kind in range(6):
            step = (1e-5, 1e-3, 0.25)[kind % 3]
            lo = np.concatenate([[0.001], np.full(d, 1e-4), [rng.uniform(1.0, 9.0)], [0.0]])
            hi = np.concatenate([[1.0], np.full(d, lo[d + 1]), [lo[d + 1] * 3.0], [1.0]])
            w = lo + rng.random(P) * (hi - lo)
            where = rng.integers(0, 6, size=P) if kind else np.zeros(P, dtype=np.int64)
            w = np.where(where == 1, lo, w)                  # on the lower bound: the lower point is clipped to it
            w = np.where(where == 2, hi, w)
            w = np.where(where == 3, lo + step / 2, w)       # half a step inside: one side clipped
            w = np.where(where == 4, hi - step / 2, w)
            w = np.minimum(np.maximum(w, lo), hi)
            val = rng.standard_normal(1 + 2 * P) * 10.0 ** rng.integers(-3, 4, size=1 + 2 * P)
            if kind >= 2:
                bad = rng.choice(1 + 2 * P, size=min(4, 1 + 2 * P), replace=False)
                val[bad] = np.array([np.nan, np.inf, -np.inf, np.nan])[:bad.size]
            if kind == 5:
                val[0] = np.nan
            out.append((d, step, w, lo, hi, val))
    return out


def _numpy(d, step, w, lo, hi, val):
    """cgp._fit_sets.evaluate for one start, with the values given: (device rows [R, 2 d + 2], f, g [P])."""
    P = d + 3
    W = w[None]
    up = np.minimum(W + step, hi[None])
    dn = np.maximum(W - step, lo[None])
    pts = np.repeat(W[:, None, :], 1 + 2 * P, axis=1)
    for j in range(P):
        pts[:, 1 + 2 * j, j] = up[:, j]
        pts[:, 2 + 2 * j, j] = dn[:, j]
    rows = cgp.rows_from_ww(pts.reshape(-1, P))
    f = np.where(np.isfinite(val), val, cgp.NONFINITE).reshape(1, 1 + 2 * P)
    with np.errstate(all="ignore"):
        g = (f[:, 1::2] - f[:, 2::2]) / (up - dn)
    return rows, float(f[0, 0]), g[0]


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_header_is_numpys_evaluate(flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe, inp = str(tmp_path / "cgp_fit_logic_check"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-I", CSRC, SRC,
                    "-o", exe], check=True)
    cases = _cases()
    with open(inp, "w") as fh:
        fh.write("%d\n" % len(cases))
        for d, step, w, lo, hi, val in cases:
            fh.write("%d %s\n%s\n%s\n%s\n%s\n" % (d, float(step).hex(), _hex(w), _hex(lo), _hex(hi), _hex(val)))
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    at = 0
    seen = dict(clipped_lo=0, clipped_hi=0, nonfinite=0, rows=0)
    for d, step, w, lo, hi, val in cases:
        P, R = d + 3, 1 + 2 * (d + 3)
        rows, f, g = _numpy(d, step, w, lo, hi, val)
        got_rows = np.array([[float.fromhex(t) for t in lines[at + r_].split()] for r_ in range(R)])
        assert got_rows.shape == (R, 2 * d + 2)
        assert got_rows.tobytes() == rows.tobytes(), (d, step)
        assert lines[at + R].split()[0] == "f" and float.fromhex(lines[at + R].split()[1]).hex() == f.hex(), (d, step)
        gl = lines[at + R + 1].split()
        assert gl[0] == "g"
        got_g = np.array([float.fromhex(t) for t in gl[1:]])
        assert got_g.shape == (P,) and np.isfinite(got_g).all()
        assert got_g.tobytes() == g.tobytes(), (d, step, got_g, g)
        at += R + 2
        seen["clipped_lo"] += int(np.sum(w - step < lo))
        seen["clipped_hi"] += int(np.sum(w + step > hi))
        seen["nonfinite"] += int(np.sum(~np.isfinite(val)))
        seen["rows"] += R
    assert at == len(lines) - 1
    print(seen)
    assert seen["clipped_lo"] > 20 and seen["clipped_hi"] > 20 and seen["nonfinite"] > 50


def test_rows_count():
    from ccgp_amd import api
    assert [api.cgp_fit_rows(d) for d in (1, 2, 9, 61)] == [9, 11, 25, 129]
    assert api.lib().ccgp_cgp_fit_rows(0) == -1
