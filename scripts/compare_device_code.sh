#!/bin/bash
# Proves that a refactor left the device code alone: compares, kernel by kernel, the gfx950 code of two source trees.
#
# usage: bash scripts/compare_device_code.sh A_DIR B_DIR
#   A_DIR, B_DIR: a csrc/ directory of *.hip units (compiled here, device side only, with the Makefile's code generation flags; warnings off), or a
#   directory of already compiled *.co files (kept by an earlier run: set KEEP=dir to keep this run's under dir/A and dir/B)
#
# Per kernel symbol it compares the disassembly (llvm-objdump -d --no-show-raw-insn --no-leading-addr) and the whole
# metadata entry (llvm-readelf --notes: VGPR / AGPR / SGPR counts, LDS, scratch, spills, the argument layout).  The kernel
# may sit in a different unit on the two sides; it may not sit in two units of one side.  Exit status 0: same set of
# kernels, every one identical.
set -e
set -o pipefail
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
[ $# -eq 2 ] || { sed -n 2,6p "$0"; exit 2; }
TMP=${KEEP:-$(mktemp -d)}
[ -n "$KEEP" ] || trap 'rm -rf "$TMP"' EXIT

compile_one() {   # unit.hip out_dir  (run inside the csrc directory; the units whose Makefile line sets -ffp-contract=off are built without FMA contraction)
    local contract=fast
    grep -Eq "^${1%.hip}\.o:[[:space:]]*CXXFLAGS[[:space:]]*:=.*-ffp-contract=off" Makefile 2> /dev/null && contract=off
    $HIPCC -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=$contract -w -I../../include -I. \
        --cuda-device-only --no-gpu-bundle-output -c "$1" -o "$2/${1%.hip}.co"
}
export -f compile_one
export HIPCC

prepare() {   # dir tag -> directory with the .co files
    if ls "$1"/*.hip > /dev/null 2>&1; then
        mkdir -p "$TMP/$2"
        ( cd "$1" && ls *.hip | xargs -P "${JOBS:-8}" -I{} bash -c "compile_one {} '$TMP/$2'" )
        echo "$TMP/$2"
    else
        echo "$1"
    fi
}
A=$(prepare "$1" A)
B=$(prepare "$2" B)

python3 - "$A" "$B" "$LLVM" <<'EOF'
import glob, os, re, subprocess, sys

def kernels(d, llvm):
    """kernel symbol -> (unit, disassembly text, metadata text); exits on a kernel that sits in two units"""
    out = {}
    for co in sorted(glob.glob(os.path.join(d, "*.co"))):
        unit = os.path.basename(co)[:-3]
        notes = subprocess.run([llvm + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        meta = {}
        for entry in re.split(r"\n  - (?=\.)", notes.split("amdhsa.kernels:")[1].split("\namdhsa.")[0] if "amdhsa.kernels:" in notes else ""):
            m = re.search(r"\.name:\s+(\S+)", entry)
            if m:
                meta[m.group(1).strip("'\"")] = entry.strip()
        dis = subprocess.run([llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                             text=True).stdout
        # symbol -> first address behind it: the zero bytes that align the next function decode as instructions under this label
        syms = subprocess.run([llvm + "/llvm-readelf", "-sW", co], check=True, capture_output=True, text=True).stdout
        end = {f[7]: int(f[1], 16) + int(f[2]) for f in (l.split() for l in syms.split("\n")) if len(f) == 8 and f[3] == "FUNC"}
        code, cur = {}, None
        for line in dis.split("\n"):
            m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
            if m:
                cur = m.group(1)
                code[cur] = []
            elif cur is not None and line.strip() != "...":      # ("...": a run of zero bytes elided, padding behind the unit's last function)
                at =re.search(r"//\s*([0-9A-Fa-f]+):", line)      # (the comment column holds the absolute address: used, then dropped)
                if at is None or int(at.group(1), 16) < end[cur]:
                    code[cur].append(re.sub(r"\s*//.*$", "", line).rstrip())
        for name, md in meta.items():
            if name in out:
                sys.exit(f"FAIL: kernel {name} is in two units of {d}: {out[name][0]} and {unit}")
            out[name] = (unit, "\n".join(code.get(name, ["<no code>"])).strip(), md)
    return out

a, b = kernels(sys.argv[1], sys.argv[3]), kernels(sys.argv[2], sys.argv[3])
bad = 0
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print(f"ONLY IN {'A' if name in a else 'B'} ({(a.get(name) or b.get(name))[0]}): {name}")
        bad += 1
        continue
    what = [w for w, i in (("instructions", 1), ("metadata", 2)) if a[name][i] != b[name][i]]
    if what:
        print(f"DIFFERENT {' and '.join(what)} ({a[name][0]} -> {b[name][0]}): {name}")
        bad += 1
moved = sum(1 for n in a if n in b and a[n][0] != b[n][0])
insns = sum(len(v[1].split("\n")) for v in a.values())
print(f"{len(a)} kernels in A, {len(b)} in B, {moved} in another unit, {insns} lines of A's disassembly compared: " + ("IDENTICAL" if bad == 0 else f"{bad} DIFFER"))
sys.exit(1 if bad else 0)
EOF
