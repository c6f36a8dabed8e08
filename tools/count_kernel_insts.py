#!/usr/bin/env python3
"""Static figures of the kernels in a gfx950 assembly listing (hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only):
instructions between a kernel's label and its end (out-of-line functions it calls are not part of it), how many of them
are 64-bit MADs, 64-bit shifts and 32-bit ANDs, and the register / scratch / spill figures of its metadata entry.

  python3 tools/count_kernel_insts.py k_ec.s [name-fragment ...]      # demangled-name fragments; default: every kernel
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    path, frags = sys.argv[1], sys.argv[2:]
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for ln in lines:            # the amdhsa.kernels metadata: one "- .agpr_count:" .. block per kernel
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", ln)
        if not m:
            continue
        k, v = m.groups()
        if ln.lstrip().startswith("- ") and k in ("agpr_count", "args"):
            cur = {}
        if cur is not None:
            cur[k] = v
            if k == "name":
                meta[v] = cur
    body, name = {}, None
    for ln in lines:
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in meta:
            name = m.group(1)
            body[name] = []
            continue
        if name and ln.startswith(".Lfunc_end"):
            name = None
            continue
        if name and re.match(r"^\t[a-z]\w+", ln):
            body[name].append(ln.split()[0])
    dm = demangle(list(body))
    print(f"{'kernel':60s} {'insts':>6s} {'mad64':>6s} {'shr64':>6s} {'and32':>6s} {'vgpr':>5s} {'agpr':>5s} {'scratch':>8s} {'spill':>6s}")
    for n, ins in body.items():
        d = re.sub(r"^void ", "", dm[n]).split("(")[0]
        if frags and not any(f in d for f in frags):
            continue
        md = meta[n]
        print(f"{d[:60]:60s} {len(ins):6d} {ins.count('v_mad_i64_i32'):6d} {ins.count('v_ashrrev_i64'):6d} {ins.count('v_and_b32_e32') + ins.count('v_and_b32'):6d} "
              f"{md.get('vgpr_count', '?'):>5s} {md.get('agpr_count', '?'):>5s} {md.get('private_segment_fixed_size', '?'):>8s} {md.get('vgpr_spill_count', '?'):>6s}")


if __name__ == "__main__":
    main()
