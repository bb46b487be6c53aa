# same-box: launch-per-phase (sched 0) against the scheduler (1: two workgroups per CU, 2: one) over the chunk size
OUT=${1:-build_ab/r05f}
mkdir -p $OUT
for B in 8 16 32 64 96 128 192 256 384; do for S in 0 1 2; do
timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-secondary --evals-total $B --steps 6 --warmup 2 --sched $S > $OUT/b${B}_s$S.json 2> $OUT/b${B}_s$S.err || { echo FAILED $B $S; exit 1; }
python - $B $S "$OUT" <<'PY'
import sys, json
B, S, out = sys.argv[1:4]
d = json.loads(open("%s/b%s_s%s.json" % (out, B, S)).read().strip().splitlines()[-1])
print("B=%s sched=%s ms/step %.2f notiming %.2f" % (B, S, d["ms_per_step"], d["notiming_ms_per_step"]), {k: round(v, 2) for k, v in d["kernel_ms_per_step"].items()}, d["config"]["matches_cpu_potrf_digest"], flush=True)
PY
done; done
