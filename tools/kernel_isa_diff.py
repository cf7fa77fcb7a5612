#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  Compares the device assembly that `make asm` (eggshell_amd/csrc)
writes for two trees, kernel by kernel, wherever a kernel lives on either side: a kernel that moved to another file,
was renamed or lost a template parameter still matches if its instructions are the same.

Each side pools the kernels of all its .s files.  A kernel's body is normalised -- comments, directives and blank
lines go, a mangled symbol becomes a placeholder, the .LBB labels are renumbered in their order of definition inside
the function; everything else, registers included, stays verbatim -- and the bodies of the two sides are matched as
multisets.  One line per kernel: "identical to <old name>" or "no match"; an unmatched kernel also gets both sides'
register counts, scratch and static LDS from the metadata, and a short unified diff against the nearest old kernel
(the one with the most lines in common, then the closer name; old kernels without a partner come first).  Exit status
1 if anything is unmatched on either side.

usage: tools/kernel_isa_diff.py OLD_DIR NEW_DIR [--only GLOB]      (GLOB: on the mangled kernel names, both sides)"""
import argparse
import collections
import difflib
import fnmatch
import glob
import os
import re
import sys

SYMBOL = re.compile(r"_Z[\w$.]+")
LABEL_DEF = re.compile(r"^([.\w$]+):")
BLOCK_LABEL = re.compile(r"\.LBB\d+_\d+")
META_KEY = re.compile(r"^(?:  - |    )(\.\w+):\s*(\S*)")
META_SHOWN = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def metadata(lines):
    """{kernel name: {key: value}} from the amdhsa.kernels list of one file."""
    out, entry, inside = {}, None, False
    for line in lines:
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):   # the next top-level key of the document
            break
        if line.startswith("  - "):
            entry = {}
        m = META_KEY.match(line)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                out[m.group(2)] = entry
    return out


def normalise(body):
    """The instructions and labels of one function, one per entry."""
    kept = []
    for line in body:
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith(".") and not LABEL_DEF.match(line):
            continue   # a directive
        kept.append(line)
    order = {}
    for line in kept:
        m = LABEL_DEF.match(line)
        if m and BLOCK_LABEL.fullmatch(m.group(1)):
            order.setdefault(m.group(1), ".LBB_%d" % len(order))
    return [SYMBOL.sub("<symbol>", BLOCK_LABEL.sub(lambda m: order.get(m.group(0), m.group(0)), line)) for line in kept]


def kernels(directory, only):
    """{kernel name: (file, normalised body, metadata)} of every .s file of a directory."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        with open(path) as fh:
            lines = fh.read().split("\n")
        meta = metadata(lines)
        name, start = None, 0
        for i, line in enumerate(lines):
            m = LABEL_DEF.match(line)
            if m and m.group(1) in meta:
                name, start = m.group(1), i + 1
            elif name and line.startswith(".Lfunc_end"):
                if only is None or fnmatch.fnmatchcase(name, only):
                    out[name] = (os.path.basename(path), normalise(lines[start:i]), meta[name])
                name = None
    return out


def compare(old, new, out=None):
    """Prints the report; returns how many kernels of either side found no partner."""
    pool = {}
    for name in sorted(old):
        pool.setdefault(tuple(old[name][1]), []).append(name)
    order = sorted(new, key=lambda n: (new[n][0], n))
    partner = {}
    for name in order:
        same = pool.get(tuple(new[name][1]))
        if same:
            partner[name] = same.pop(same.index(name) if name in same else 0)
    left = [n for names in pool.values() for n in names]   # old kernels without a partner: the likely counterparts
    unmatched = 0
    for name in order:
        f, body, meta = new[name]
        if name in partner:
            print("%s: %s: identical to %s: %s" % (f, name, old[partner[name]][0], partner[name]), file=out)
            continue
        unmatched += 1
        print("%s: %s: no match" % (f, name), file=out)
        # the nearest old kernel: a name says little across a rename, so the one with the most lines in common, of those
        # without a partner if there are any; the closer name decides between equals
        lines = collections.Counter(body)
        near = sorted(left or old, key=lambda o: (-sum((lines & collections.Counter(old[o][1])).values()),
                                                  -difflib.SequenceMatcher(None, name, o).ratio()))[:1]
        show = lambda m: ", ".join("%s %s" % (k, m.get(k, "?")) for k in META_SHOWN)
        print("    new: %s" % show(meta), file=out)
        if near:
            print("    old: %s   (nearest: %s: %s)" % (show(old[near[0]][2]), old[near[0]][0], near[0]), file=out)
            diff = list(difflib.unified_diff(old[near[0]][1], body, "old", "new", n=2, lineterm=""))
            for line in diff[:40]:
                print("    " + line, file=out)
            if len(diff) > 40:
                print("    ... %d more lines" % (len(diff) - 40), file=out)
    for names in pool.values():
        for name in names:
            unmatched += 1
            print("%s: %s: no match (on the old side only)" % (old[name][0], name), file=out)
    print("%d kernels old, %d new, %d without a partner" % (len(old), len(new), unmatched), file=out)
    return unmatched


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--only", metavar="GLOB", default=None)
    a = ap.parse_args(argv)
    return 1 if compare(kernels(a.old_dir, a.only), kernels(a.new_dir, a.only)) else 0


if __name__ == "__main__":
    sys.exit(main())
