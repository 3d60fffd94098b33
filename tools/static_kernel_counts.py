#!/usr/bin/env python3
"""Whole-kernel static counts of step-kernel instantiations in a product-build `make asm` listing: branch instructions by kind,
exec-mask saves, scalar multiplies, instruction lines, registers and spills.  What a change to the common path is read against
BEFORE the GPU is asked (the dynamic counts are tools/pmc_roles.sh's).

    make -C sequential_social_dilemma_games_amd/csrc asm
    python tools/static_kernel_counts.py csrc/ssd_kernels.s [mangled-name-substring ...]

Default kernels: the coherent map-specific step kernels of the headline (Harvest 16x38, 5 agents), of Cleanup 25x18 with 5 and
10 agents and of Cleanup 48x36 with 10.
"""
import re
import sys

DEFAULT = [("harvest n5", "ILi0ELi0ELb0ELi5ELb1ELi1ELb1ELb0E"), ("cleanup n5", "ILi1ELi0ELb0ELi5ELb1ELi1ELb1ELb0E"),
           ("cleanup n10", "ILi1ELi0ELb0ELi10ELb1ELi1ELb1ELb0E"), ("cleanup48x36 n10", "ILi1ELi0ELb0ELi10ELb1ELi2ELb1ELb0E")]
KINDS = ["s_cbranch_vcc", "s_cbranch_scc", "s_cbranch_exec", "s_branch"]


def count(lines, sub):
    start = [k for k, l in enumerate(lines) if l.startswith("_ZN3ssd14ssd_env_kernel") and sub in l and ":" in l][0]
    c = {k: 0 for k in KINDS}
    c.update(saveexec=0, s_mul=0, lines=0, valu=0, salu=0, lds=0, vmem=0, smem=0)
    end = start
    for end in range(start + 1, len(lines)):
        l = lines[end]
        if l.startswith(".Lfunc_end"):
            break
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        c["lines"] += 1
        for k in KINDS:
            if op.startswith(k):
                c[k] += 1
        if "saveexec" in op:
            c["saveexec"] += 1
        if op.startswith("s_mul"):
            c["s_mul"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            c["smem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_")):
            c["vmem"] += 1
        elif op.startswith("s_") and not op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop")):
            c["salu"] += 1
    meta = {}
    for l in lines[end:end + 60]:
        m = re.match(r";\s*(TotalNumSgprs|NumVgprs|ScratchSize|Occupancy):\s*(\d+)", l.strip())
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return c, meta


def main():
    lines = open(sys.argv[1]).read().split("\n")
    which = [(s, s) for s in sys.argv[2:]] or DEFAULT
    for name, sub in which:
        c, meta = count(lines, sub)
        print("%s  (%s)" % (name, sub))
        print("  lines %d   branches %d: " % (c["lines"], sum(c[k] for k in KINDS)) + "  ".join("%s* %d" % (k, c[k]) for k in KINDS))
        print("  saveexec %d   s_mul* %d   valu %d  salu %d  lds %d  vmem %d  smem %d" %
              (c["saveexec"], c["s_mul"], c["valu"], c["salu"], c["lds"], c["vmem"], c["smem"]))
        print("  VGPR %s  SGPR %s  scratch bytes (spills) %s  occupancy %s" %
              (meta.get("NumVgprs"), meta.get("TotalNumSgprs"), meta.get("ScratchSize"), meta.get("Occupancy")))


if __name__ == "__main__":
    main()
