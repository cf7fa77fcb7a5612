#!/usr/bin/env python3
"""Are the barrier loops of one kernel the same in two builds?  For a kernel whose prologue or epilogue changed,
tools/kernel_isa_diff.py reports "no match" and a diff of the whole body, in which scalar registers renumbered by the
changed prologue drown everything else.  This tool finds the kernel's loops in the assembly of `make asm` -- the blocks
the compiler's own annotations put innermost in one loop, in text order -- keeps those that hold an s_barrier (a
timetable loop: every block of steps ends in one; a loop nested in it, which has none, is left out of it on both
sides) and matches them between the two builds as
multisets, twice: the opcodes alone, and the instructions with their vector registers verbatim and every scalar
register and block label masked (a renumbered SGPR is the same instruction sequence).  One line per loop of the new
build: its size, its fp64 VALU instructions, and whether the old build has the same loop.  Exit status 1 if a loop has
no partner under either comparison, or the builds differ in the number of such loops.

usage: tools/kernel_loop_diff.py OLD.s NEW.s KERNEL_SUBSTRING"""
import collections
import re
import sys

SGPR = re.compile(r"\bs\[\d+:\d+\]|\bs\d+\b|\bvcc\b|\bttmp\d+\b")
LABEL = re.compile(r"\.LBB\d+_\d+")
F64 = re.compile(r"^v_\w+_f64")
BB_MARK = re.compile(r"%bb\.\d+:")
HEADER = re.compile(r"Header=(BB\d+_\d+)")


def barrier_loops(path, name):
    """The innermost loops with a barrier (lists of instructions) of the first function whose symbol contains `name`."""
    # the compiler says of every block which loop it is innermost in: "in Loop: Header=BB0_35 Depth=2" behind the
    # block's label (or its "; %bb.N:" marker), "This Inner Loop Header" / "This Loop Header" behind or below a header's
    loops, cur, last, inside = collections.OrderedDict(), None, None, False
    for line in open(path):
        text, _, note = line.partition(";")
        text = text.strip()
        if not inside:
            if text.endswith(":") and name in text and not text.startswith("."):
                inside = True
            continue
        if text.startswith(".Lfunc_end"):
            break
        block = text[:-1].lstrip(".L") if text.endswith(":") else BB_MARK.match(note.strip()) and "%bb"
        if block:
            last = block
            member = HEADER.search(note)
            cur = member.group(1) if member else None
        if "Loop Header: Depth" in note:
            cur = last
        if text and not text.startswith(".") and not text.endswith(":") and cur:
            loops.setdefault(cur, []).append(text)
    return [b for b in loops.values() if any(i.startswith("s_barrier") for i in b)]


def key(loop, masked):
    if masked:
        return tuple(LABEL.sub(".L", SGPR.sub("s#", i)) for i in loop)
    return tuple(i.split()[0] for i in loop)


def main():
    if len(sys.argv) != 4:
        sys.exit(__doc__)
    old, new = barrier_loops(sys.argv[1], sys.argv[3]), barrier_loops(sys.argv[2], sys.argv[3])
    print("%s: %d innermost loops with a barrier in the old build, %d in the new" % (sys.argv[3], len(old), len(new)))
    if not old or not new:
        print("    none found: wrong kernel name?")
        return 1
    bad = len(old) != len(new)
    left = {m: collections.Counter(key(b, m) for b in old) for m in (False, True)}
    for n, b in enumerate(new):
        found = {}
        for m in (False, True):
            found[m] = left[m][key(b, m)] > 0
            if found[m]:
                left[m][key(b, m)] -= 1
        print("    loop %d: %4d instructions, %3d fp64 VALU, %d barrier(s): opcodes %s; instructions with scalar registers masked %s" % (
            n, len(b), sum(1 for i in b if F64.match(i)), sum(1 for i in b if i.startswith("s_barrier")),
            "identical" if found[False] else "NO PARTNER", "identical" if found[True] else "NO PARTNER"))
        bad |= not (found[False] and found[True])
        if not found[False]:   # the same instructions in another order?  The old loop nearest in its opcode counts
            mine = collections.Counter(i.split()[0] for i in b)
            diff = min(({op: (c[op], mine[op]) for op in set(c) | set(mine) if c[op] != mine[op]}
                        for c in (collections.Counter(i.split()[0] for i in o) for o in old)), key=len)
            print("        opcode counts against the nearest old loop (old, new): %s" % (diff or "the same: another order"))
    return int(bad)


if __name__ == "__main__":
    sys.exit(main())
