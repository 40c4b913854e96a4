#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel.

    compare_kernel_text.py PARENT_DIR NEW_DIR [--only STEM ...]

Each directory holds the *.s files that `hipcc ... -save-temps=obj -c x.hip -o DIR/x.o` leaves for the device side
(x-hip-amdgcn-amd-amdhsa-gfx950.s), built with the Makefile's flags.  For every kernel of the parent's files (all of them, or those of
the source files named with --only, e.g. `--only xs_integrate`) the script asks that

  * the symbol exists in exactly one file of the new build,
  * its text is identical: the lines from its label to its .Lfunc_end, without comments, blank lines and the .loc / .file / .cfi
    directives.  One thing is normalised: local labels carry the function's ordinal in its file (.LBB7_12, .Lfunc_end7), which
    changes when a kernel moves to another file or another place in its file; the ordinal is dropped (.LBB_12),
  * .vgpr_count, .sgpr_count, .private_segment_fixed_size and .group_segment_fixed_size of its metadata entry are identical.

Prints one line per kernel and exits 1 if any kernel differs or is missing.  It compares text; it searches for nothing.
"""
import difflib
import glob
import os
import re
import sys

FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
ORDINAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")
DROP = re.compile(r"^\s*\.(loc|file|cfi_\w+)\b")


def device_files(d, only):
    files = sorted(glob.glob(os.path.join(d, "*-hip-amdgcn-amd-amdhsa-*.s")))
    if only:
        files = [f for f in files if os.path.basename(f).split("-hip-amdgcn")[0] in only]
    return files


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    if not line.strip() or DROP.match(line):
        return None
    return ORDINAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def kernels_of(path):
    """{symbol: (text lines, {figure: value})} of one device assembly file"""
    lines = open(path).read().split("\n")
    figures, name, cur = {}, None, {}
    in_meta = False
    for ln in lines:
        s = ln.strip()
        if s == "amdhsa.kernels:":
            in_meta = True
            continue
        if not in_meta:
            continue
        if s.startswith("- ") and not ln.startswith("      "):   # a new kernel entry of the list
            if name:
                figures[name] = cur
            name, cur = None, {}
            s = s[2:].strip()
        elif not (ln.startswith("    .") or s.startswith("amdhsa.")):   # an argument's own fields
            continue
        key, _, val = s.partition(":")
        if key == ".name":
            name = val.strip()
        elif key in FIGURES:
            cur[key] = val.strip()
        if s.startswith("amdhsa.target"):
            break
    if name:
        figures[name] = cur
    out = {}
    for sym in figures:
        try:
            b = lines.index(sym + ":") if sym + ":" in lines else next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        except StopIteration:
            continue
        e = next(i for i in range(b, len(lines)) if lines[i].startswith(".Lfunc_end"))
        out[sym] = ([c for c in map(clean, lines[b:e + 1]) if c is not None], figures[sym])
    return out


def main(argv):
    only = []
    if "--only" in argv:
        i = argv.index("--only")
        only, argv = argv[i + 1:], argv[:i]
    if len(argv) != 3:
        sys.exit(__doc__)
    parent, new = {}, {}
    for f in device_files(argv[1], only):
        parent.update(kernels_of(f))
    where = {}
    for f in device_files(argv[2], []):
        for sym, v in kernels_of(f).items():
            where.setdefault(sym, []).append(os.path.basename(f).split("-hip-amdgcn")[0])
            new[sym] = v
    bad = 0
    for sym, (text, fig) in parent.items():
        figs = " ".join("%s %s" % (k[1:], fig.get(k, "?")) for k in FIGURES)
        if len(where.get(sym, [])) != 1:
            verdict = "MISSING" if sym not in where else "IN %d FILES" % len(where[sym])
        else:
            ntext, nfig = new[sym]
            if ntext != text:
                n = sum(1 for d in difflib.unified_diff(text, ntext, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                verdict = "TEXT DIFFERS (%d of %d lines)" % (n, len(text))
            elif nfig != fig:
                verdict = "FIGURES DIFFER (%s)" % nfig
            else:
                verdict = "identical (%d lines, now in %s)" % (len(text), where[sym][0])
        bad += not verdict.startswith("identical")
        print("%s  %s  %s" % (sym, figs, verdict))
    print("%d kernels, %d not identical" % (len(parent), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
