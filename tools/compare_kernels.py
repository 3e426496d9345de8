"""Machine-code identity of two builds of libfpq_hip.so, on the CPU: every kernel of the second build must carry the same
instruction stream and the same register / LDS / scratch figures as in the first.

usage: compare_kernels.py BEFORE.so AFTER.so [--rename 'REGEX=>REPLACEMENT' ...] [--allow-reorder]

The gfx950 code objects are taken out of each library's .hip_fatbin section as tests/test_no_spill.py does
(llvm-objcopy, clang-offload-bundler), every kernel symbol is disassembled (llvm-objdump -d --no-show-raw-insn) with
addresses, branch-target comments and symbol offsets stripped, and kernels are matched by their demangled names.  A
--rename rule maps a demangled name of BEFORE to the name the kernel carries in AFTER (a template parameter dropped).
Prints the kernel counts, the kernels that disappeared or appeared (by template name), and every kernel whose code or
figures differ; exit status 1 if any do.  --allow-reorder: a kernel with equal figures whose instructions are the same
multiset in another order (the scheduler's answer to a moved source line) is reported as REORDERED with the size of its
diff and does not fail the run."""
import argparse
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIGURES = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    elfs = []
    for k, a in enumerate(starts):
        b = starts[k + 1] if k + 1 < len(starts) else len(data)
        bundle, elf = os.path.join(tmp, f"bundle{k}"), os.path.join(tmp, f"co{k}.elf")
        open(bundle, "wb").write(data[a:b])
        subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={bundle}", f"--output={elf}"], check=True)
        elfs.append(elf)
    return elfs


def figures(elf):
    """{mangled kernel name: {figure: value}} from the code object's metadata notes"""
    notes = subprocess.run([tool("llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    recs, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if key == "agpr_count" and (cur is None or "agpr_count" in cur):   # first key of a kernel's record
            cur = {}
            recs.append(cur)
        if cur is not None:
            cur[key] = val
    return {r["name"]: {f: r.get(f) for f in FIGURES} for r in recs if "name" in r}


def data_symbols(elf):
    """[(start, end, name)] of the code object's data symbols, and [(start, end, name)] of its sections"""
    syms = subprocess.run([tool("llvm-readelf"), "-s", "--wide", elf], check=True, capture_output=True, text=True).stdout
    out = set()
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "OBJECT" and f[0].endswith(":"):
            out.add((int(f[1], 16), int(f[1], 16) + int(f[2], 0), f[7]))
    secs = subprocess.run([tool("llvm-readelf"), "-S", "--wide", elf], check=True, capture_output=True, text=True).stdout
    sections = []
    for line in secs.splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", line)
        if m and int(m.group(2), 16):
            sections.append((int(m.group(2), 16), int(m.group(2), 16) + int(m.group(3), 16), m.group(1)))
    return sorted(out), sections


def where(addr, syms, sections):
    for a, b, name in syms:
        if a <= addr < b:
            return f"{name}+{addr - a}"
    for a, b, name in sections:   # no symbol: the section and the offset in it
        if a <= addr < b:
            return f"{name}+{addr - a}"
    return f"?{addr:#x}"


def disassembly(elf, kernels):
    """{mangled kernel name: [normalised instruction lines]}.  The PC-relative address of s_getpc_b64 + s_add_u32 +
    s_addc_u32 (global data: tables, the option block) is replaced by the data symbol and offset it resolves to, since
    where the data lies moves with the code around it."""
    text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", elf], check=True, capture_output=True,
                          text=True).stdout
    syms, sections = data_symbols(elf)
    out, cur, pc, lo = {}, None, {}, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in kernels else None
            if cur is not None:
                out[cur] = []
            pc, lo = {}, {}
            continue
        if cur is None or not line.strip():
            continue
        am = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        ins = re.sub(r"//.*$", "", line).strip()            # address / encoding comments
        ins = re.sub(r"<[^>]*>", "", ins).strip()            # symbol+offset annotations
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", ins)
        if m and am:
            pc[int(m.group(1))] = int(am.group(1), 16) + 4
        m = re.match(r"s_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins)
        if m and m.group(1) == m.group(2) and int(m.group(1)) in pc:
            r = int(m.group(1))
            lo[r + 1] = (pc.pop(r), int(m.group(3), 0) & 0xFFFFFFFF, len(out[cur]))
            ins = f"s_add_u32 s{r}, s{r}, @pcrel"
        m = re.match(r"s_addc_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", ins)
        if m and m.group(1) == m.group(2) and int(m.group(1)) in lo:
            base, low, at = lo.pop(int(m.group(1)))
            target = (base + ((int(m.group(3), 0) & 0xFFFFFFFF) << 32 | low)) & (2**64 - 1)
            out[cur][at] += " " + where(target, syms, sections)
            ins = f"s_addc_u32 s{m.group(1)}, s{m.group(1)}, @pcrel"
        if ins:
            out[cur].append(ins)
    for ins in out.values():   # "..." after the last instruction: the zero fill up to the next symbol, which moves with the layout
        while ins and ins[-1] == "...":
            ins.pop()
    return out


def demangle(names):
    """{mangled: demangled}; _Float16 (DF16_) is passed to the demangler as `half` (Dh), which older ones read too"""
    filt = tool("llvm-cxxfilt") or shutil.which("c++filt")
    res = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for n in names), check=True, capture_output=True,
                         text=True).stdout
    return {n: d.replace("half", "_Float16").replace("(anonymous namespace)::", "") for n, d in zip(names, res.splitlines())}


def load(lib, tmp):
    kernels = {}
    for elf in code_objects(lib, tmp):
        fig = figures(elf)
        dis = disassembly(elf, set(fig))
        for name, f in fig.items():
            kernels[name] = (f, dis.get(name))
    dem = demangle(sorted(kernels))
    return {dem[n]: v for n, v in kernels.items()}


def template_name(demangled):
    return re.split(r"[<(]", demangled, maxsplit=1)[0].split()[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[], help="'REGEX=>REPLACEMENT' on the demangled names of BEFORE")
    ap.add_argument("--list", action="store_true", help="print every kernel that disappeared or appeared")
    ap.add_argument("--allow-reorder", action="store_true", help="equal figures and equal sorted instructions: REORDERED, not a failure")
    args = ap.parse_args()
    rules = [(re.compile(r.split("=>")[0]), r.split("=>")[1]) for r in args.rename]
    with tempfile.TemporaryDirectory() as tb, tempfile.TemporaryDirectory() as ta:
        before, after = load(args.before, tb), load(args.after, ta)
    renamed = {}
    for name in before:
        new = name
        for rx, rep in rules:
            new = rx.sub(rep, new)
        renamed[name] = new
    by_new = {v: k for k, v in renamed.items()}
    assert len(by_new) == len(renamed), "the --rename rules map two kernels to one name"
    gone = sorted(n for n in before if renamed[n] not in after)
    new = sorted(n for n in after if n not in by_new)
    print(f"kernels: {len(before)} before, {len(after)} after")
    for title, names in (("disappeared", gone), ("appeared", new)):
        counts = collections.Counter(template_name(n) for n in names)
        print(f"{title}: {len(names)}" + "".join(f"\n  {c:4d}  {t}" for t, c in sorted(counts.items())))
        if args.list:
            for n in names:
                print(f"    {n}")
    moved = [(o, n) for o, n in renamed.items() if o != n and n in after]
    if moved:
        print(f"renamed: {len(moved)}")
        for o, n in sorted(moved):
            print(f"  {o}\n    -> {n}")
    bad = reordered = 0
    for old, name in sorted(renamed.items()):
        if name not in after:
            continue
        (fb, db), (fa, da) = before[old], after[name]
        if fb != fa:
            bad += 1
            print(f"FIGURES DIFFER {name}: {fb} -> {fa}")
        if args.allow_reorder and fb == fa and db and da and db != da and sorted(db) == sorted(da):
            reordered += 1
            moved_lines = [d for d in difflib.unified_diff(db, da, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---")]
            print(f"REORDERED {name}: {len(db)} instructions, {len(moved_lines)} diff lines: " + "; ".join(sorted(set(d[1:] for d in moved_lines))))
        elif db is None or da is None or db != da:
            bad += 1
            print(f"CODE DIFFERS {name}: {len(db or [])} -> {len(da or [])} instructions")
    kept = len(before) - len(gone)
    print((f"identical: {kept - bad - reordered} of {kept} kept kernels" if not bad else f"{bad} differences among {kept} kept kernels") +
          (f", reordered: {reordered}" if args.allow_reorder else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
