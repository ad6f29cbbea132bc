#!/usr/bin/env python3
"""Do two sets of device code objects hold the same kernels?  One line per kernel symbol.

    hipcc $(FLAGS) --offload-device-only --no-gpu-bundle-output -c X.hip -o X.co -Rpass-analysis=kernel-resource-usage 2> X.co.log
    compare_kernel_code.py --old old/flow_kernels.co --new new/flow_prep.co new/flow_level.co ...

Per kernel (every STT_FUNC symbol with a .kd descriptor beside it) it compares the code size (llvm-readelf -sW), the resource report of the
compiler's remarks (X.co.log beside X.co: SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS ...) and the disassembly with addresses stripped.
Exit status 1 if any kernel differs or exists on one side only.
"""
import argparse, os, re, shutil, subprocess, sys

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def sizes(co):
    syms, kds = {}, set()
    for line in run(f"{LLVM}/llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            syms[f[7]] = int(f[2])
        elif len(f) == 8 and f[7].endswith(".kd"):
            kds.add(f[7][:-3])
    return {k: v for k, v in syms.items() if k in kds}


def resources(co):
    out, cur = {}, None
    if not os.path.exists(co + ".log"):
        return out
    for line in open(co + ".log"):
        m = re.search(r"remark:\s*(Function Name|[A-Za-z][A-Za-z /\[\]]*?): (\S+)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), [])
        elif cur is not None:
            cur.append(f"{m.group(1).strip()}={m.group(2)}")
    return {k: " ".join(v) for k, v in out.items()}


def disassembly(co, size):
    out, cur, end = {}, None, 0
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:$", line)
        a = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if m:
            cur, end = out.setdefault(m.group(2), []), int(m.group(1), 16) + size.get(m.group(2), 0)
        elif cur is not None and a and int(a.group(1), 16) < end:      # (what follows a function's last byte is padding up to the next symbol)
            cur.append(re.sub(r"\s*//.*$", "", line).strip())          # the address comment and the branch-target label go; branch offsets are relative and stay
    return out


def gather(files):
    S, R, D, where = {}, {}, {}, {}
    for co in files:
        s = sizes(co)
        for k in s:
            where[k] = os.path.basename(co)
        S.update(s); R.update(resources(co)); D.update({k: v for k, v in disassembly(co, s).items() if k in s})
    return S, R, D, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    So, Ro, Do, Wo = gather(a.old)
    Sn, Rn, Dn, Wn = gather(a.new)
    bad = 0
    names = sorted(set(So) | set(Sn))
    filt = next((f for f in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt")) if f and os.path.exists(f)), None)
    demangle = dict(zip(names, run(filt, *names).splitlines())) if filt else {k: k for k in names}
    for k in sorted(names, key=lambda k: demangle[k]):
        name = demangle[k].split("(")[0]
        if k not in So or k not in Sn:
            print(f"{name}: ONLY IN {'old ' + Wo[k] if k in So else 'new ' + Wn[k]}"); bad += 1; continue
        size = "same" if So[k] == Sn[k] else f"{So[k]} -> {Sn[k]}"
        res = "no report" if k not in Ro or k not in Rn else "same" if Ro[k] == Rn[k] else f"[{Ro[k]}] -> [{Rn[k]}]"
        ndiff = sum(1 for x, y in zip(Do[k], Dn[k]) if x != y) + abs(len(Do[k]) - len(Dn[k]))
        dis = "same" if ndiff == 0 else f"{ndiff} lines differ"
        ok = size == "same" and res == "same" and dis == "same"
        bad += 0 if ok else 1
        print(f"{name}: {Wo[k]} -> {Wn[k]}  size {So[k]} B {size}; resources {res} ({Rn.get(k, '')}); disassembly {len(Dn[k])} lines {dis}")
    print(f"{len(names)} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
