#!/usr/bin/env python3
"""diff_device_asm.py OLD.s NEW.s [--map old=new ...] -- are two device listings the same code, function by function?

For a refactor of kernel source that must not move the code: compile the unit before and after with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -S --cuda-device-only [-D...] csrc/msm.hip -o X.s
(the flags of count_isa.py) and compare.  Per function of OLD: the instruction stream (mnemonics and operands; comments, directives
and label lines dropped, the function number taken out of .LBB labels) and the resources .amdhsa_next_free_vgpr / _sgpr, the LDS
size and ScratchSize.  A function that was renamed is matched through --map; each side is a mangled symbol or a piece of one that
fits exactly one function (`bucket_sum_heavy_pairs=bucket_sum_heavyINS_9PairLanes`), and the same renaming is applied to symbol operands
(the callee of a call sequence).  One line per function: `identical`, or the first differing instruction and the resource
changes; functions only NEW has are listed.  Exit status 1 when anything differs.  It only diffs: nothing is said about WHICH
instructions appear.  No GPU needed."""
import argparse
import re
import sys

RESOURCES = {"vgpr": r"\.amdhsa_next_free_vgpr\s+(.+)", "sgpr": r"\.amdhsa_next_free_sgpr\s+(.+)",
             "lds": r"\.amdhsa_group_segment_fixed_size\s+(.+)", "scratch": r"; ScratchSize:\s*(\d+)"}


def functions(path):
    """{symbol: (instructions, resources)} of a listing; a function's region runs from its .type line to the next one."""
    out, name, in_body = {}, None, False
    for ln in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name, in_body = m.group(1), False
            out[name] = ([], {})
            continue
        if name is None:
            continue
        s = ln.strip()
        if s.startswith(name + ":"):
            in_body = True
        elif s.startswith(".Lfunc_end"):
            in_body = False
        elif in_body and s and s[0] not in ";." and not re.match(r"\S+:", s):
            out[name][0].append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split(";")[0].split())))
        for key, pat in RESOURCES.items():
            m = re.search(pat, s)
            if m and key not in out[name][1]:
                out[name][1][key] = m.group(1).strip()
    return out


def resolve(piece, names, side):
    hits = [piece] if piece in names else [n for n in names if piece in n]
    if len(hits) != 1:
        sys.exit("diff_device_asm: --map %s '%s' fits %d functions of %s" % (side, piece, len(hits), side))
    return hits[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    old, new = functions(args.old), functions(args.new)
    rename = {}
    for pair in args.map:
        a, b = pair.split("=", 1)
        rename[resolve(a, old, "OLD")] = resolve(b, new, "NEW")

    def renamed(text):                                   # longest symbol first: one symbol may be the head of another
        for a in sorted(rename, key=len, reverse=True):
            text = text.replace(a, rename[a])
        return text

    differ = 0
    for name, (ins, res) in old.items():
        target = rename.get(name, name)
        label = name if target == name else "%s -> %s" % (name, target)
        if target not in new:
            print("%s: MISSING in NEW" % label)
            differ += 1
            continue
        ins2, res2 = new[target]
        ins = [renamed(i) for i in ins]
        notes = ["%s %s -> %s" % (k, renamed(res.get(k, "-")), res2.get(k, "-")) for k in RESOURCES if renamed(res.get(k, "-")) != res2.get(k, "-")]
        first = next((i for i, (a, b) in enumerate(zip(ins, ins2)) if a != b), None)
        if first is None and len(ins) != len(ins2):
            first = min(len(ins), len(ins2))
        if first is not None:
            notes.insert(0, "instruction %d of %d / %d: `%s` -> `%s`" % (first, len(ins), len(ins2), (ins + ["<end>"])[first], (ins2 + ["<end>"])[first]))
        print("%s: %s" % (label, "; ".join(notes) if notes else "identical (%d instructions)" % len(ins)))
        differ += bool(notes)
    for name in new:
        if name not in old and name not in rename.values():
            print("%s: only in NEW" % name)
            differ += 1
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
