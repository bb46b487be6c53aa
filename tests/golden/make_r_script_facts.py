#!/usr/bin/env python3
"""Generate tests/golden/r_script_facts.json: what r/ccgp.R and r/ccgp_shim.c assume about the eight reference R scripts,
read off those scripts once.

tests/test_r_wrappers_vs_reference.py checks the wrappers against this record, so the suite needs no copy of the
scripts (and none is kept: the record holds argument lists, column names, counts and the yes / no answers of the
pattern checks, never script text).

Run from the repo root with a checkout of the reference repository:
    python tests/golden/make_r_script_facts.py <reference checkout>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SCRIPTS = {
    "HX": "Heat Exchanger Emulator/Combined GP Heat Exchanger.R",
    "GV": "Ground Vibrations Emulator/Combined GP Ground Vibrations.R",
    "ISO": "2D Codes and Designs/2D Combined GP Isotropic Public.R",
    "ADV": "2D Codes and Designs/2D Combined GP Isotropic Advanced.R",
    "ANI": "2D Codes and Designs/2D Combined GP Anisotropic Public.R",
    "BSQ": "Batch Sequential ME Designs/Batch Sequential ME Design.R",
    "D1": "1D Codes and Designs/1D Combined GP Public.R",
    "D1F": "1D Codes and Designs/1D Combined GP Two Families Public.R",
}
METRO_SCRIPTS = ("HX", "GV", "ISO", "ADV", "ANI", "BSQ")


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


def prediction_facts(src):
    _, body = definition(src, "prediction")
    return {
        "apply_over_frame_calls": len(re.findall(r"apply\s*\(\s*pars\.frame\s*,\s*1\s*,\s*predict\.post", body)),
        "apply_calls": len(re.findall(r"\bapply\s*\(", body)),
        "returns_transposed_mean_var_frame": bool(re.search(r"data\.frame\s*\(\s*t\s*\(\s*apply", body)
                                                  and re.search(r'c\("mean",\s*"var"\)', body)),
    }


def factors_frame_facts(src):
    _, body = definition(src, "factors.frame")
    m = re.search(r'names\(samp\)\s*<-\s*c\(([^)]*)\)', body)
    return {
        "samp_columns": [c.strip().strip('"') for c in m.group(1).split(",")],
        "returns_samp_beta_factors_rinv": bool(re.search(
            r"return\s*\(\s*cbind\s*\(\s*samp\s*,\s*beta\s*,\s*prediction\.factors\s*,\s*R\.Inv\s*\)\s*\)", body)),
        "passes_n_train_y_train_to_factors": bool(re.search(
            r"factors\s*,\s*n\.train\s*=\s*n\.train\s*,\s*y\.train\s*=\s*y\.train", body.replace("\n", " "))),
    }


def predict_post_facts(tag, src):
    _, body = definition(src, "predict.post")
    m = re.search(r"beta\s*<-\s*as\.numeric\(pars\[(\d+)\]\)", body)
    out = {"beta_column": int(m.group(1)) if m else None}
    if tag == "ADV":
        m = re.search(r"lambda\s*<-\s*as\.numeric\(pars\[(\d+)\]\)", body)
        out["lambda_column"] = int(m.group(1)) if m else None
        out["scales_theta1_by_one_plus_lambda"] = "theta1*(1+lambda)" in body.replace(" ", "")
    return out


def metro_facts(tag, src):
    _, body = definition(src, "Metro")
    flat = re.sub(r"\s+", "", body)
    i_u = flat.find("u<-runif(1)")
    i_c = flat.find("theta.candidate<-rmnorm(1,as.vector(theta.old),sqrt(2)*pars$v)")
    tail = "R.Inv=R.Inv[(k-samp.size):(k-1)]" + (",logpost=log.posterior[(k-samp.size):(k-1)]" if tag == "BSQ" else "") + "))"
    by_position = True
    for m in re.finditer(r"\bMetro\s*\(([^)]*)\)", src):
        if "function" in src[max(0, m.start() - 12):m.start()]:
            continue
        by_position = by_position and "=" not in m.group(1)
    return {
        # one uniform, then one multivariate-normal candidate per iteration, in this order, and no other draw
        "draws_runif_then_rmnorm_only": (0 < i_u < i_c and flat.count("runif(") == 1 and flat.count("rmnorm(") == 1
                                         and "rnorm(" not in flat.replace("rmnorm(", "")),
        "accepts_on_log_ratio": "R<-l.cand$val-l.old$val" in flat and "if(R>log(u))" in flat,
        "loops_while_k_le_N_and_pv_lt_alpha": "while(k<=N&pv<alpha)" in flat,
        "geweke_every_batch_after_samp_size": "if((k-1)>=samp.size&(k-1)%%batch.size==0)" in flat,
        "geweke_on_last_samp_size_draws": "geweke.diag(mcmc(samp[(k-samp.size):(k-1)]))$z" in flat,
        "starts_from_laplace_mode": (("est<-laplace(logpost.val,start)" in flat or "est<-laplace(logpost.val,start,...)" in flat)
                                     and "pars<-list(mu=est$mode,v=est$var)" in flat
                                     and "theta.old<-pars$mu" in flat and "k=1" in flat),
        "returns_last_samp_size_with_rinv": flat.rstrip("}").endswith(tail),
        "every_call_passes_arguments_by_position": by_position,
    }


def main(ref):
    facts = {}
    for tag, rel in sorted(SCRIPTS.items()):
        with open(os.path.join(ref, rel), encoding="latin-1") as fh:
            src = fh.read()
        formals = {}
        for fn in ("compare.GP", "prediction", "factors.frame", "logpost", "factors", "predict.post", "Metro"):
            d = definition(src, fn)
            formals[fn] = d[0] if d is not None else None
        rec = {"formals": formals, "prediction": prediction_facts(src), "factors.frame": factors_frame_facts(src),
               "predict.post": predict_post_facts(tag, src)}
        if tag in METRO_SCRIPTS:
            rec["Metro"] = metro_facts(tag, src)
        facts[tag] = rec
    path = os.path.join(HERE, "r_script_facts.json")
    with open(path, "w") as fh:
        json.dump(facts, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
