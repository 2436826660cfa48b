#!/usr/bin/env python3
"""Condense hipcc's `-Rpass-analysis=kernel-resource-usage` remarks into one line per kernel, and compare two builds.

    hipcc ... -Rpass-analysis=kernel-resource-usage ... 2> build.log
    scripts/resource_usage.py table build.log [name-filter ...]      # kernel, SGPRs, VGPRs, scratch, occupancy, LDS
    scripts/resource_usage.py diff parent.log head.log [name-filter ...]

`diff` prints the kernels present in both logs whose VGPRs, scratch or occupancy differ, then the kernels only the second
log has, and exits 1 when a common kernel differs.  Kernel names are demangled with c++filt when it is on the PATH."""
import re
import shutil
import subprocess
import sys

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"),
          ("LDS Size [bytes/block]", "lds"))


def parse(path):
    out, cur = {}, None
    with open(path, errors="replace") as f:
        for line in f:
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            if cur is None:
                continue
            for label, key in FIELDS:
                m = re.search(r"remark:\s+" + re.escape(label) + r": (\S+)", line)
                if m and key not in cur:
                    cur[key] = int(m.group(1))
    return out


def demangle(names):
    if not names or not shutil.which("c++filt"):
        return {n: n for n in names}
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    short = []
    for line in res.stdout.splitlines():
        line = re.sub(r"^void ", "", line).replace("(anonymous namespace)::", "")
        short.append(re.sub(r"\(.*$", "", line))  # template arguments kept, the parameter list dropped
    return dict(zip(names, short))


def row(name, r):
    return (f"{name:<58} sgpr {r.get('sgpr', -1):>3} vgpr {r.get('vgpr', -1):>3} scratch {r.get('scratch', -1):>4} "
            f"occ {r.get('occ', -1)} spill {r.get('sspill', 0)}/{r.get('vspill', 0)} lds {r.get('lds', 0)}")


def main(argv):
    if len(argv) < 3 or argv[1] not in ("table", "diff"):
        sys.exit(__doc__)
    if argv[1] == "table":
        tab, filt = parse(argv[2]), argv[3:]
        names = demangle(sorted(tab))
        for n in sorted(tab, key=lambda n: names[n]):
            if not filt or any(f in names[n] for f in filt):
                print(row(names[n], tab[n]))
        return 0
    a, b, filt = parse(argv[2]), parse(argv[3]), argv[4:]
    names = demangle(sorted(set(a) | set(b)))
    keep = lambda n: not filt or any(f in names[n] for f in filt)
    common = [n for n in sorted(a, key=lambda n: names[n]) if n in b and keep(n)]
    moved = [n for n in common if any(a[n].get(k) != b[n].get(k) for k in ("vgpr", "scratch", "occ"))]
    print(f"{len(common)} kernels in both builds, {len(moved)} with other VGPRs / scratch / occupancy")
    for n in moved:
        print("- " + row(names[n], a[n]))
        print("+ " + row(names[n], b[n]))
    new = [n for n in sorted(b, key=lambda n: names[n]) if n not in a and keep(n)]
    print(f"{len(new)} kernels only in the second build")
    for n in new:
        print("  " + row(names[n], b[n]))
    gone = [names[n] for n in a if n not in b and keep(n)]
    if gone:
        print("only in the first build: " + ", ".join(sorted(gone)))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
