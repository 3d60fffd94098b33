#!/usr/bin/env python3
"""tools/ab_libs.py OUT REPS LABEL=LIB [LABEL=LIB ...] -- bench-args...  -- on the GPU box: ab_lib.sh for more than two libraries.
bench.py --no-extras [args] with each library in turn (SSD_LIB_PATH; LIB "-" = the product library), alternating fresh processes on
the same box, REPS rounds; us per step of each run, then median, range and half-range per label, appended to OUT."""
import json, os, subprocess, sys
out, reps = sys.argv[1], int(sys.argv[2])
rest = sys.argv[3:]
sep = rest.index("--")
libs = [a.split("=", 1) for a in rest[:sep]]
bargs = rest[sep + 1:]
res = {k: [] for k, _ in libs}
with open(out, "a") as f:
    f.write("# bench.py --no-extras %s ; alternating fresh processes, %d rounds; us per step\n" % (" ".join(bargs), reps))
    for r in range(reps):
        for k, lib in libs:
            env = dict(os.environ)
            env.pop("SSD_LIB_PATH", None)
            if lib != "-":
                env["SSD_LIB_PATH"] = os.path.abspath(lib)
            p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "bench.py", "--no-extras"] + bargs, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            if p.returncode != 0:
                f.write("FAILED rc=%d lib=%s\n" % (p.returncode, lib)); f.flush()
                print("FAILED", p.returncode, lib); sys.exit(p.returncode or 1)
            d = json.loads(p.stdout.decode().strip().splitlines()[-1])
            v = round(d["ms_per_step"] * 1e3, 3)
            res[k].append(v)
            f.write("%s %.3f\n" % (k, v)); f.flush()
            print(k, v, flush=True)
    for k, _ in libs:
        v = sorted(res[k])
        line = "%s median %.3f min %.3f max %.3f half-range %.3f" % (k, v[len(v) // 2], v[0], v[-1], (v[-1] - v[0]) / 2)
        f.write(line + "\n"); print(line)
