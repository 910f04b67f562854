#!/usr/bin/env python3
"""Register / spill / instruction-mix table of every kernel in libfmri_hip.so, from the code objects' own metadata and
disassembly (llvm-readelf --notes, llvm-objdump -d).  Dev container or GPU box; writes plain text to stdout.

usage: tools/isa_report.py [path/to/libfmri_hip.so] > profiles/rNN_isa.txt
       tools/isa_report.py --diff OLD.so NEW.so      (per kernel: identical, or what changed; exit status 1 on a change)
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_store_hazard as ssh     # noqa: E402  (code-object extraction)

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FILT = "c++filt"
FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size"]
COUNT = [("mfma", r"v_mfma_"), ("readlane", r"v_readlane_b32"), ("writelane", r"v_writelane_b32"),
         ("scratch", r"scratch_(load|store)"), ("s_nop", r"s_nop"), ("waitcnt", r"s_waitcnt"), ("barrier", r"s_barrier")]


def short(name):
    m = re.match(r"_ZN4fmri(\d+)", name)          # (c++filt does not know the _Float16 mangling: keep the bare name)
    if m:
        n0 = m.end()
        name = name[n0:n0 + int(m.group(1))] + ("<" + ",".join(re.findall(r"Li(\d+)E", name)) + ">" if "ILi" in name else "")
    name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", ""))
    return name.replace("void ", "").replace("fmri::", "")


def collect(lib):
    """[(mangled name, metadata, instruction counts, instruction lines without addresses and labels)] of a library."""
    tmp, objs = ssh.code_objects(lib)
    rows = []
    try:
        for o in objs:
            notes = subprocess.run([READELF, "--notes", o], check=True, capture_output=True, text=True).stdout
            meta = {}
            for blk in notes.split("\n  - .agpr_count:")[1:]:
                blk = ".agpr_count:" + blk
                nm = re.search(r"\.name:\s+(\S+)", blk)
                if not nm:
                    continue
                meta[nm.group(1)] = {f: int(m.group(1)) if (m := re.search(re.escape(f) + r":\s+(\d+)", blk)) else 0 for f in FIELDS}
            dis = subprocess.run([ssh.OBJDUMP, "-d", "--no-show-raw-insn", o], check=True, capture_output=True, text=True).stdout
            cur, counts, text = None, {}, {}
            for line in dis.splitlines():
                lm = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if lm:
                    cur = lm.group(1) if lm.group(1) in meta else cur
                    counts.setdefault(cur, {k: 0 for k, _ in COUNT} | {"instr": 0})
                    continue
                if cur is None or not line.strip() or line.lstrip().startswith((";", ".")):
                    continue
                c = counts[cur]
                c["instr"] += 1
                text.setdefault(cur, []).append(line.split("//")[0].strip())
                for k, pat in COUNT:
                    if re.search(r"^\s*" + pat, line):
                        c[k] += 1
            for k, m in meta.items():
                rows.append((k, m, counts.get(k, {}), text.get(k, [])))
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
    return rows


def demangled(rows):
    return subprocess.run([FILT], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()


def diff(old_lib, new_lib):
    """Per kernel of two builds: identical, or the metadata / instruction-mix columns that changed (old -> new) and the
    number of differing instruction lines.  Addresses and labels are not compared (branches are relative), and the
    per-translation-unit __hip_cuid_* symbol is data, not kernel text."""
    import difflib
    old, new = ({r[0]: r for r in collect(lib)} for lib in (old_lib, new_lib))
    names = dict(zip(new, demangled(list(new.values())))) | dict(zip(old, demangled(list(old.values()))))
    print(f"# {os.path.basename(old_lib)} -> {os.path.basename(new_lib)}: {len(old)} -> {len(new)} kernels")
    changed = 0
    for k in sorted(set(old) | set(new), key=lambda k: short(names[k])):
        if k not in old or k not in new:
            what = "only in " + ("NEW" if k in new else "OLD")
        elif old[k][1:] == new[k][1:]:
            what = "identical"
        else:
            (_, mo, co, to), (_, mn, cn, tn) = old[k], new[k]
            cols = [f"{f.strip('.')} {a[f]} -> {b[f]}" for a, b in ((mo, mn), (co, cn)) for f in a if a[f] != b.get(f)]
            nlines = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in
                         difflib.SequenceMatcher(None, to, tn, autojunk=False).get_opcodes() if tag != "equal")
            what = f"CHANGED: {nlines} of {len(to)} instruction lines differ" + "".join("; " + c for c in cols)
        changed += what != "identical"
        print(f"{short(names[k])[:58]:58s} {what}")
    print(f"# {changed} kernels changed")
    return 1 if changed else 0


def main(argv):
    if argv and argv[0] == "--diff":
        return diff(argv[1], argv[2])
    here = os.path.dirname(os.path.abspath(__file__))
    lib = argv[0] if argv else os.path.join(here, "..", "thesis-fmri-reconstruction_amd", "fmri_hip", "libfmri_hip.so")
    rows = collect(lib)
    names = demangled(rows)
    print("# libfmri_hip.so: per-kernel registers, spills and instruction mix (code-object metadata + disassembly)")
    print(f"{'kernel':58s} {'vgpr':>4s} {'agpr':>4s} {'sgpr':>4s} {'vspill':>6s} {'sspill':>6s} {'scratchB':>8s} {'ldsB':>6s} "
          f"{'instr':>6s} {'mfma':>5s} {'rdlane':>6s} {'wrlane':>6s} {'scr.ops':>7s} {'s_nop':>5s} {'barrier':>7s}")
    for (k, m, c, _), nm in sorted(zip(rows, names), key=lambda t: -t[0][2].get("mfma", 0)):
        print(f"{short(nm)[:58]:58s} {m['.vgpr_count']:4d} {m['.agpr_count']:4d} {m['.sgpr_count']:4d} {m['.vgpr_spill_count']:6d} "
              f"{m['.sgpr_spill_count']:6d} {m['.private_segment_fixed_size']:8d} {m['.group_segment_fixed_size']:6d} "
              f"{c.get('instr', 0):6d} {c.get('mfma', 0):5d} {c.get('readlane', 0):6d} {c.get('writelane', 0):6d} "
              f"{c.get('scratch', 0):7d} {c.get('s_nop', 0):5d} {c.get('barrier', 0):7d}")


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
