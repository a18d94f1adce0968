#!/usr/bin/env python3
"""Prints `kernel-name hash` for every gfx950 kernel of csrc/*.hip, sorted by name: sha256 over the kernel's function body and
its .amdhsa_kernel descriptor block, compiled with the flags of build.py plus `--cuda-device-only -S`.  Two trees compute the same
device code exactly when `diff` finds their two lists equal -- the check of a refactor that moves kernels between translation units.

What depends on a kernel's position in its unit is normalised away: the `__hip_cuid_` lines, the unit-wide numbering of local labels
(`.LBB<n>_<m>` -> `.LBB_<m>`, also where a comment names a loop header `BB<n>_<m>`; `.Lfunc_end<n>`, `.LJTI<n>_<m>`, `.Ltmp<n>`), `.file` / `.loc` / `.ident` lines.

    tools/kernel_isa.py [--asm DIR] [--parts] [extra hipcc flags, e.g. -DTGNH_TRACE]     (--asm keeps the assembly files in DIR)

--parts prints two more hashes per kernel, of the descriptor block alone and of the body's sorted opcodes: two kernels that differ
in the first hash and agree in these two hold the same instructions under the same resources in another order.
"""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "openmm_drudenose_amd", "csrc")
args = sys.argv[1:]
keep = args.pop(args.index("--asm") + 1) if "--asm" in args else None
parts = "--parts" in args
args = [a for a in args if a not in ("--asm", "--parts")]


def normalise(line):
    line = re.sub(r"(\.L|\b)(BB|JTI)\d+_(\d+)", r"\1\2_\3", line)          # labels, and the loop headers named in comments
    line = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", line)
    return " ".join(line.split()) + "\n"                                  # (a comment's column follows the label's length)


def kernels(asm):
    """{kernel: hash} of one assembly file"""
    body, desc, cur, in_desc, functions = {}, {}, None, None, set()
    for line in open(asm):
        if "__hip_cuid_" in line or re.match(r"\s+\.(file|loc|ident|cv_file|cv_loc)\b", line):
            continue
        m = re.match(r"\s+\.type\s+(\w+),@function", line)
        if m: functions.add(m.group(1))
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in functions:                 # (a variable's label opens nothing)
            cur = m.group(1); body[cur] = []
        m = re.match(r"\s+\.amdhsa_kernel\s+(\w+)", line)
        if m:
            in_desc = m.group(1); desc[in_desc] = []
        if cur: body[cur].append(normalise(line))
        if in_desc: desc[in_desc].append(normalise(line))
        if cur and re.match(r"^\.Lfunc_end\d+:", line): cur = None
        if in_desc and ".end_amdhsa_kernel" in line: in_desc = None
    sha = lambda lines: hashlib.sha256("".join(lines).encode()).hexdigest()[:16]
    if not parts:
        return {k: sha(body[k] + desc[k]) for k in desc}
    # an instruction: an indented line that is neither a directive nor a comment; its opcode is the first word
    opcodes = lambda lines: sorted(l.split()[0] + "\n" for l in lines if l[:1] not in ".;" and not re.match(r"^[\w.$]+:", l) and l.strip())
    return {k: " ".join([sha(body[k] + desc[k]), sha(desc[k]), sha(opcodes(body[k]))]) for k in desc}


def compile_one(name, tmp):
    asm = os.path.join(tmp, name + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-S",
                    os.path.join(csrc, name), "-o", asm] + args, check=True)
    return kernels(asm)


with tempfile.TemporaryDirectory() as tmp:
    tmp = keep or tmp
    os.makedirs(tmp, exist_ok=True)
    units = sorted(n for n in os.listdir(csrc) if n.endswith(".hip"))
    with ThreadPoolExecutor(len(units)) as pool:
        found = list(pool.map(lambda n: compile_one(n, tmp), units))
for unit, ks in zip(units, found):
    print(f"# {unit}: {len(ks)} kernels", file=sys.stderr)
for name, h in sorted((k, h) for ks in found for k, h in ks.items()):
    print(name, h)
