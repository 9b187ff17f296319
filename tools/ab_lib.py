#!/usr/bin/env python3
"""Same-session A/B of two builds of the library on bench.py lines (alternating, so that box drift shows):
    python tools/ab_lib.py <base.so> <new.so> [rounds] [short|c2] [record.txt]
short (default): per round and build, `bench.py` for C4 / C2 / C5 inverse and C4 / C2 forward (no CPU leg, no PMC);
prints ms_per_step, the last lines are the medians.
c2: the lines of profiles/r07_c2_contig_p4_ab.txt and r08_c2_range_schedule_ab.txt -- c2, c5, the C2 call at batch 1022
(tools/c2_batch1022.py) and c2 inverse, 400 timed calls after 50 -- with the sha256 of both libraries, and at the end the
verdict lines of the project's rule: the mean must improve by more than 3 x the larger within-build range.  Stops at the
first run that fails.  record.txt: a copy of everything printed."""
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
base, new = sys.argv[1], sys.argv[2]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
which = sys.argv[4] if len(sys.argv) > 4 else "short"
record = open(sys.argv[5], "w") if len(sys.argv) > 5 else None
BENCH = [sys.executable, os.path.join(ROOT, "bench.py")]
COMMON = ["--no-traffic", "--no-cpu-baseline", "--no-power", "--no-other-configs", "--no-shard-overheads"]
LONG = ["--steps", "400", "--warmup", "50", "--no-e2e"]
LINE_SETS = {
    "short": (("c4_inv", BENCH + ["--config", "c4", "--direction", "inv", "--steps", "50", "--warmup", "10"] + COMMON),
              ("c4_fwd", BENCH + ["--config", "c4", "--steps", "50", "--warmup", "10"] + COMMON),
              ("c2_inv", BENCH + ["--direction", "inv", "--steps", "20", "--warmup", "5"] + COMMON),
              ("c2_fwd", BENCH + ["--steps", "20", "--warmup", "5"] + COMMON),
              ("c5_inv", BENCH + ["--config", "c5", "--direction", "inv", "--steps", "20", "--warmup", "5"] + COMMON)),
    "c2": (("c2", BENCH + LONG + COMMON),
           ("c5", BENCH + ["--config", "c5"] + LONG + COMMON),
           ("c2_b1022", [sys.executable, os.path.join(ROOT, "tools", "c2_batch1022.py")]),
           ("c2_inv", BENCH + ["--direction", "inv"] + LONG + COMMON)),
}
LINES = LINE_SETS[which]
BUILDS = (("base", base), ("new", new)) if which == "short" else (("parent", base), ("new", new))


def say(text):
    print(text, flush=True)
    if record:
        record.write(text + "\n")
        record.flush()


if which != "short":
    for tag, so in BUILDS:
        with open(so, "rb") as f:
            say("# sha256 %s %s" % (tag, hashlib.sha256(f.read()).hexdigest()))
res = {}
for r in range(rounds):
    for tag, so in BUILDS:
        for name, cmd in LINES:
            out = subprocess.run(cmd, env=dict(os.environ, GPUNTT_LIB=os.path.abspath(so)), capture_output=True, text=True)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or not line:
                say("%s %s FAILED rc=%d %s" % (tag, name, out.returncode, out.stderr[-300:]))
                if which != "short":
                    sys.exit(1)
                continue
            d = json.loads(line[-1])
            ok = d.get("batch_check", {}).get("bit_exact", d.get("cpu_baseline", {}).get("gpu_output_bit_exact"))
            res.setdefault((name, tag), []).append(d["ms_per_step"])
            if which == "short":
                say("round %d %-5s %-7s %.4f ms  check=%s" % (r, tag, name, d["ms_per_step"], ok))
            else:
                say("rep %d %-6s %-8s ms_per_step %.5f check=%s" % (r, tag, name, d["ms_per_step"], ok))
if which == "short":
    say("medians (ms per call):")
    for name, _ in LINES:
        b, n = statistics.median(res[(name, "base")]), statistics.median(res[(name, "new")])
        say("  %-7s base %.4f  new %.4f  (%+.1f %%)" % (name, b, n, 100 * (n / b - 1)))
else:
    say("## verdict (rule: the mean must improve by more than 3 x the larger within-build range of the repetitions)")
    for name, _ in LINES:
        b, n = res[(name, "parent")], res[(name, "new")]
        mb, mn = statistics.mean(b), statistics.mean(n)
        rb, rn = max(b) - min(b), max(n) - min(n)
        say("# %-8s parent mean %.5f ms (range %.5f)   new mean %.5f ms (range %.5f)   %+.5f ms = %+.1f %%   3 x range = %.5f"
            % (name, mb, rb, mn, rn, mn - mb, 100 * (mn / mb - 1), 3 * max(rb, rn)))
