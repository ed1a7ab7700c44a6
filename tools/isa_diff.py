"""Device-code comparison of two builds of the library: which kernels are instruction-equal, which changed, which are gone.

    python tools/isa_diff.py OLD_BUILD_DIR NEW_BUILD_DIR        (the directories that hold the *.hip.o of build.py)

Every kernel is reduced to its instruction stream (mnemonics and operands as `llvm-objdump -d` prints them; branch operands are relative
already, addresses and symbol names are dropped) and matched BY STREAM + resources (VGPRs, SGPRs, LDS bytes, scratch bytes), not by name -
dropping a template parameter changes the mangled name and nothing else.  Kernels of the new build without such a partner are paired with
the old kernel of the closest demangled name and printed with both sets of figures.

Limits: `s_nop` padding is not part of a stream, so kernels that differ only in it count as equal (neither is the `...` llvm-objdump prints
for a run of zero bytes: the alignment gap behind a kernel's `s_endpgm`, which depends on what the code object holds next); the pairing of a changed kernel with an old
one is by name similarity alone (it can pair unrelated kernels) - read the "was" line of every pair.  A kernel of the new build for which no old
kernel of the same template name is left over is printed as new, with its own figures."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_lint  # noqa: E402

META = ("name", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(co):
    """-> {mangled name: (vgpr, sgpr, lds, scratch, (instruction, ...))}"""
    tool = lambda *a: subprocess.run([os.path.join(isa_lint.LLVM, a[0])] + list(a[1:]), capture_output=True, text=True, check=True).stdout
    meta, cur = {}, {}
    for ln in tool("llvm-readelf", "--notes", co).split("\n"):
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- .") and ln.index("-") < 6:      # first key of a kernel record (argument records are nested deeper)
            cur = {}
        if m.group(1) in META:
            cur[m.group(1)] = m.group(2)
            if len(cur) == len(META):
                meta[cur["name"]] = tuple(int(cur[k]) for k in META[1:])
    out, name = {}, None
    for ln in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            name = m.group(1) if m.group(1) in meta else None
            if name:
                out[name] = []
            continue
        t = re.sub(r"\s+", " ", ln.partition("//")[0]).strip()
        if name and t and not t.startswith("s_nop") and not t.startswith("s_code_end") and t != "...":
            out[name].append(t)
    return {n: meta[n] + (tuple(ins),) for n, ins in out.items()}


def load(build_dir):
    ks = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(build_dir)):
            if f.endswith(".hip.o"):
                co = isa_lint.code_object(os.path.join(build_dir, f), tmp)
                if co:
                    ks.update(kernels(co))
    return ks


_FILT = next((t for t in (os.path.join(isa_lint.LLVM, "llvm-cxxfilt"), "/usr/bin/c++filt") if os.path.exists(t)), None)
_SHORT = {}


def short(name):
    if name in _SHORT:
        return _SHORT[name]
    d = (subprocess.run([_FILT, name], capture_output=True, text=True).stdout.strip() if _FILT else "") or name
    _SHORT[name] = re.sub(r"\(.*", "", d.replace("void ", "").replace("wis::", "").replace("(anonymous namespace)::", ""))
    return _SHORT[name]


def waves(vgpr):
    return min(8, 512 // (((vgpr + 7) // 8) * 8)) if vgpr else 8


def main(old_dir, new_dir):
    old, new = load(old_dir), load(new_dir)
    pool = collections.defaultdict(list)
    for n, k in old.items():
        pool[k].append(n)
    equal, changed = [], []
    for n, k in sorted(new.items()):
        if pool[k]:
            # the same name first, so that a renamed twin does not take it
            equal.append((n, pool[k].pop(pool[k].index(n) if n in pool[k] else 0)))
        else:
            changed.append(n)
    left = sorted(n for ns in pool.values() for n in ns)
    gone = list(left)
    # (a kernel the old build has no like of - no old kernel left over that shares the name in front of the template arguments - is new)
    fresh = [n for n in changed if not any(short(g).split("<")[0] == short(n).split("<")[0] for g in gone)]
    print(f"kernels: {len(old)} old, {len(new)} new; {len(equal)} instruction-equal with equal VGPRs / SGPRs / LDS / scratch "
          f"({sum(1 for a, b in equal if a != b)} of them under a new name), {len(changed) - len(fresh)} changed, {len(fresh)} added, "
          f"{len(left) - len(changed) + len(fresh)} gone")
    print("\n## changed (old -> new): instructions, VGPRs, SGPRs, LDS bytes, scratch bytes, waves per SIMD by registers")
    for n in changed:
        if n in fresh:
            b = new[n]
            print(f"{short(n)}\n    new: instr {len(b[4])}, VGPR {b[0]}, SGPR {b[1]}, LDS {b[2]}, scratch {b[3]}")
            continue
        cand = difflib.get_close_matches(short(n), [short(g) for g in gone], n=1, cutoff=0.0)
        o = next(g for g in gone if short(g) == cand[0])
        gone.remove(o)
        a, b = old[o], new[n]
        sm = difflib.SequenceMatcher(None, a[4], b[4], autojunk=False)
        same = sum(bl.size for bl in sm.get_matching_blocks())
        print(f"{short(n)}\n    was {short(o)}\n    instr {len(a[4])} -> {len(b[4])} ({same} in common), VGPR {a[0]} -> {b[0]}, SGPR {a[1]} -> {b[1]}, "
              f"LDS {a[2]} -> {b[2]}, scratch {a[3]} -> {b[3]}, waves {waves(a[0])} -> {waves(b[0])}")
    print("\n## gone")
    for g in gone:
        print(short(g))
    print("\n## instruction-equal under a new name")
    for a, b in equal:
        if a != b:
            print(f"{short(b)} -> {short(a)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
