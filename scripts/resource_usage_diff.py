"""Compare the compiler's per-kernel resource usage of two builds of one source file: registers, scratch, LDS, occupancy.
Input: the remark output of each build, e.g. for csrc/small_reg.hip
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c small_reg.hip -o /dev/null 2> new.txt
(`make -C csrc resource-usage` prints the same remarks) and the same command on the other tree.  Kernels are matched by
demangled name; a template argument the new build appended with its default value (`, false` at the end of
small_reg_kernel's list) is dropped for the match, so an instance that existed before is compared with itself; likewise a
kernel the new build turned into a template over switches (cgp_state_kernel<false>) matches the parent's plain kernel where
every switch is `false`, and a template over switches that gained further ones (cgp_state_kernel<true, false>) matches the
parent's instance with the leading switches (cgp_state_kernel<true>) where the added ones are `false`.  Prints every
difference, the counts, and the kernels only the new build has -- each beside the pre-existing instance with the same
leading arguments.  Needs c++filt.  Exit status 1 when a pre-existing kernel differs.
    python scripts/resource_usage_diff.py parent.txt new.txt [--appended 1]"""
import argparse
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "TotalSGPRs",
        "SGPRs Spill", "VGPRs Spill"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    """demangled names; an argument type chosen by a switch, std::conditional<false, A, B>::type, is written as the type it
    is (B), so a kernel that became a template over such a switch (cgp_predict_kernel<false>) matches the parent's plain one"""
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    cond = re.compile(r"std::conditional<(true|false), ([^<>,]+), ([^<>,]+)>::type")
    return {k: cond.sub(lambda m: m.group(2 if m.group(1) == "true" else 3), v) for k, v in zip(names, r.stdout.split("\n"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--appended", type=int, default=1, help="template arguments the new build appended to its kernels")
    args = ap.parse_args()
    par, new = parse(args.parent), parse(args.new)
    dp, dn = demangle(list(par)), demangle(list(new))
    parent_names = set(dp.values())
    nargs = {len(re.match(r".*?<([^>]*)>", v).group(1).split(",")) for v in dp.values() if "small_reg_kernel<" in v}

    def split(name):
        """(name without the appended arguments, True when they are not all `false`)"""
        # a switch appended behind non-boolean template arguments (site_corr_kernel<1, false>, predict_summary_kernel<2, true,
        # false>): the parent's instance where it is `false`, a new instance beside it where it is `true`
        m = re.match(r"(.*?<[^>]*?), (true|false)(>.*)", name)
        if m and "small_reg_kernel<" not in name and m.group(1) + m.group(3) in parent_names:
            return m.group(1) + m.group(3), m.group(2) == "true"
        # a plain kernel that became a template over one switch AND gained a last parameter for it (summary_valid_kernel<false>)
        m = re.match(r"void (.*?)<(true|false)>(\(.*), [^,()]*(?:\([^()]*\))?[^,()]*\)$", name)
        if m and m.group(1) + m.group(3) + ")" in parent_names:
            return m.group(1) + m.group(3) + ")", m.group(2) == "true"
        m = re.match(r"void (.*?)<((?:true|false)(?:, (?:true|false))*)>(\(.*)", name)
        if m and m.group(1) + m.group(3) in parent_names:   # a plain kernel of the parent that became a template over switches
            return m.group(1) + m.group(3), "true" in m.group(2)
        m = re.match(r"void (.*?)<true>(\(.*)", name)
        if m and any(v.startswith("void " + m.group(1) + "<false>(") for v in dn.values()):
            # the `true` sibling of a kernel that became a template over ONE switch, with an argument type of its own
            # (cgp_predict_kernel<true>): new, shown beside the parent's plain kernel
            base = [p for p in parent_names if p.startswith(m.group(1) + "(")]
            return (base[0] if base else name), True
        m = re.match(r"(.*?<)((?:true|false)(?:, (?:true|false))+)(>.*)", name)
        if m and "small_reg_kernel<" not in name:   # a template over switches that gained some (cgp_state_kernel's GATED)
            a = m.group(2).split(", ")
            for cut in range(1, len(a)):
                if m.group(1) + ", ".join(a[:len(a) - cut]) + m.group(3) in parent_names:
                    return m.group(1) + ", ".join(a[:len(a) - cut]) + m.group(3), "true" in a[len(a) - cut:]
        m = re.match(r"(.*?<)([^>]*)(>.*)", name)
        if not m or "small_reg_kernel<" not in name:
            return name, False
        a = [x.strip() for x in m.group(2).split(",")]
        if len(a) - args.appended not in nargs:
            return name, False
        tail = a[len(a) - args.appended:]
        return m.group(1) + ", ".join(a[:len(a) - args.appended]) + m.group(3), any(t != "false" for t in tail)

    old_form, added = {}, {}
    for k, v in dn.items():
        name, is_new = split(v)
        (added if is_new else old_form)[name] = new[k]
    differ = 0
    for k, v in dp.items():
        if v not in old_form:
            print("MISSING in the new build:", v)
            differ += 1
            continue
        for q in KEYS:
            if par[k].get(q) != old_form[v].get(q):
                print("DIFFERS %s: %s %s -> %s" % (v, q, par[k].get(q), old_form[v].get(q)))
                differ += 1
    print("kernels in the parent build: %d; compared: %d; differing figures (%s): %d; kernels only in the new build: %d" % (
        len(par), len(par), ", ".join(k.split(" [")[0] for k in KEYS), differ, len(added) + len(set(old_form) - set(dp.values()))))
    show = KEYS[:1] + KEYS[2:5]
    for name in sorted(added, key=lambda s: [int(x) for x in re.findall(r"\d+", s)] + [s]):
        base = old_form.get(name, {})
        arg = re.search(r"<([^>]*)>", name)
        print("new %s: %s" % (arg.group(1) if arg else re.search(r"(\w+)\(", name).group(1) + "<true>",
                              " | ".join("%s %s (%s)" % (q.split(" [")[0], added[name].get(q), base.get(q, "-")) for q in show)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
