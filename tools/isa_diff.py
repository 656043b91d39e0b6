#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two trees' kernel sources, kernel symbol by kernel symbol.

    python tools/isa_diff.py OLD_CSRC NEW_CSRC [-j N]

For every source of NEW_CSRC/Makefile's SRCS both trees' file is compiled device-only with the Makefile's flags and disassembled
(llvm-objdump -d --no-show-raw-insn --no-leading-addr, symbol+offset annotations removed).  Prints, per file, the kernels compared,
those present on one side only and those whose instruction text differs, then one summary line; exit status 1 if anything differs.
It diffs and does nothing else: no GPU, nothing written outside a temporary directory."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Xclang -target-feature -Xclang -packed-fp32-ops".split()


def srcs(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    return re.search(r"^SRCS\s*:=\s*(.*)$", text, re.M).group(1).split()


def kernels(csrc, src, tmp):
    """{symbol: instruction text} of one source's device code"""
    obj = os.path.join(tmp, src + ".o")
    subprocess.run([HIPCC, *FLAGS, "--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", obj], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip():
            out[name].append(re.sub(r"\s*<[^>]*>\s*$", "", re.sub(r"\s*//.*$", "", line)).strip())
    return {k: "\n".join(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    files = srcs(a.new)
    total = differing = 0
    only = []
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new, concurrent.futures.ThreadPoolExecutor(a.j) as ex:
        jobs = {f: (ex.submit(kernels, a.old, f, t_old), ex.submit(kernels, a.new, f, t_new)) for f in files}
        for f in files:
            old, new = jobs[f][0].result(), jobs[f][1].result()
            diff = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
            gone, added = sorted(old.keys() - new.keys()), sorted(new.keys() - old.keys())
            total += len(old.keys() & new.keys())
            differing += len(diff)
            only += [f"-{k}" for k in gone] + [f"+{k}" for k in added]
            print(f"{f}: {len(old.keys() & new.keys())} kernels compared, {len(diff)} differ" +
                  "".join(f"\n  differs: {k}" for k in diff) + "".join(f"\n  only old: {k}" for k in gone) + "".join(f"\n  only new: {k}" for k in added))
    print(f"files {len(files)}, kernels compared {total}, kernels differing {differing}, on one side only {len(only)}: {' '.join(only)}")
    return 1 if differing or any(o.startswith("-") for o in only) else 0


if __name__ == "__main__":
    sys.exit(main())
