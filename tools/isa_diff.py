#!/usr/bin/env python3
"""Device assembly of two source trees, file by file (no GPU): the check that a host-side change left the kernels alone.

Compiles every csrc/*.hip of each tree for gfx950 with gvamd/build.py's FLAGS plus --cuda-device-only -S, drops the
lines that differ between any two builds of one text (the __hip_cuid_* symbol, .file, .ident) and prints, per file,
`identical` or the number of differing lines.  A file only one tree has is reported as such (a rename: compare it by
hand with --pair).

    python3 tools/isa_diff.py PARENT_TREE THIS_TREE [--pair OLD.hip=NEW.hip ...] [--keep DIR] [--kernels FILE.hip ...]
                              [--moved OLD.hip=NEW.hip ...]

--kernels FILE.hip: the file is meant to differ (it gained kernels, say); print each of its gv:: kernels as identical,
differs, or only in one tree, by instruction lines.
--moved OLD.hip=NEW.hip (repeatable, one OLD may name several NEW): kernels of the parent's OLD now live in this tree's
NEW.  Every gv:: function of OLD is looked up in its NEW files and printed as `identical` or `differs (n lines)`, by its
instruction lines and by its .amdhsa_kernel descriptor block (registers, LDS, scratch); one found in no NEW file, or
in two, is printed as such.  OLD and NEW are not compared as whole files.  Two things are normalised first: the
function ordinal in basic-block labels (.LBB25_3 -> .LBB_3, at the label and where a branch names it) and the comment
behind a label.  A label is a local name: the assembler resolves it to an offset inside the function, and the ordinal
only says how many functions the file emitted before this one, which a move changes and the machine code does not see.
The comment is the compiler's note on loop nesting, padded to a column that depends on the label's length.
Exit status 0 when every compared file (but those named by --kernels) is identical and every function of a --moved OLD
is identical in exactly one NEW."""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grid-vision_amd"))
from gvamd import build as gvbuild  # noqa: E402

_VOLATILE = re.compile(r"__hip_cuid_|^\s*\.file\b|^\s*\.ident\b")


def csrc_of(tree: str) -> str:
    return os.path.join(os.path.abspath(tree), "grid-vision_amd", "csrc")


def device_asm(csrc: str, src: str, out: str) -> list:
    """The device assembly of csrc/src without the lines no two builds share."""
    cmd = [gvbuild.hipcc(), *gvbuild.FLAGS, "--cuda-device-only", "-S", "-o", out, os.path.join(csrc, src)]
    r = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise RuntimeError("compile failed: " + os.path.join(csrc, src))
    with open(out) as f:
        return [ln for ln in f.read().splitlines() if not _VOLATILE.search(ln)]


def differing_lines(a: list, b: list) -> int:
    return sum(1 for ln in difflib.unified_diff(a, b, lineterm="", n=0)
               if ln[:1] in "+-" and not ln.startswith(("+++", "---")))


def kernel_bodies(asm: list) -> dict:
    """{symbol: its instruction lines} of every gv:: function of one file's assembly, comments dropped: what --kernels
    compares when a file changed but one of its kernels must not have."""
    out, cur = {}, None
    for ln in asm:
        m = re.match(r"^(_ZN2gv\w+):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
            elif not ln.lstrip().startswith(";"):
                out[cur].append(ln)
    return out


_BB = re.compile(r"(?<=\.L)BB\d+_")
_LABEL = re.compile(r"^([.\w$]+:)\s*;.*$")


def moved_parts(asm: list) -> dict:
    """{symbol: (instruction lines, descriptor lines)} for --moved: kernel_bodies' lines with the function ordinal taken
    out of the basic-block labels and the comment behind a label dropped, the .amdhsa_kernel block apart."""
    out = {}
    for sym, lines in kernel_bodies(asm).items():
        lines = [_BB.sub("BB_", _LABEL.sub(r"\1", ln)) for ln in lines]
        k = next((i for i, ln in enumerate(lines) if ln.strip().startswith(".amdhsa_kernel")), len(lines))
        out[sym] = (lines[:k], lines[k:])
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW", help="a renamed file: parent's name = this tree's name")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files there")
    ap.add_argument("--kernels", action="append", default=[], metavar="FILE.hip",
                    help="also compare this file kernel by kernel (its differing lines then do not count for the exit status)")
    ap.add_argument("--moved", action="append", default=[], metavar="OLD=NEW",
                    help="kernels of the parent's OLD live in this tree's NEW: compare them one by one (repeatable)")
    a = ap.parse_args()
    ca, cb = csrc_of(a.parent), csrc_of(a.this)
    hips = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".hip"))   # noqa: E731
    fa, fb = hips(ca), hips(cb)
    moved = {}   # OLD -> its NEW files
    for o, n in (m.split("=", 1) for m in a.moved):
        moved.setdefault(o, []).append(n)
    moved_new = {n for ns in moved.values() for n in ns}
    pairs = [tuple(p.split("=", 1)) for p in a.pair]
    pairs += [(f, f) for f in fa if f in fb and f not in [p[0] for p in pairs] and f not in moved and f not in moved_new]
    paired_a, paired_b = {p[0] for p in pairs} | set(moved), {p[1] for p in pairs} | moved_new
    out_dir = a.keep or tempfile.mkdtemp(prefix="gv_isa_")
    os.makedirs(out_dir, exist_ok=True)
    try:
        jobs = [(ca, o, os.path.join(out_dir, "a_" + o + ".s")) for o, _ in pairs]
        jobs += [(cb, n, os.path.join(out_dir, "b_" + n + ".s")) for _, n in pairs]
        jobs += [(ca, o, os.path.join(out_dir, "a_" + o + ".s")) for o in sorted(moved)]
        jobs += [(cb, n, os.path.join(out_dir, "b_" + n + ".s")) for n in sorted(moved_new)]
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            asm = list(ex.map(lambda j: device_asm(*j), jobs))
    finally:
        if not a.keep:
            shutil.rmtree(out_dir, ignore_errors=True)
    asm_old = dict(zip(sorted(moved), asm[2 * len(pairs):]))
    asm_new = dict(zip(sorted(moved_new), asm[2 * len(pairs) + len(moved):]))
    print("flags: " + " ".join(gvbuild.FLAGS) + " --cuda-device-only -S")
    worst = 0
    for k, (o, n) in sorted(enumerate(pairs), key=lambda kp: kp[1][1]):
        d = differing_lines(asm[k], asm[len(pairs) + k])
        if n not in a.kernels:
            worst = max(worst, d)
        name = n if o == n else o + " -> " + n
        print(f"{name:44s} {'identical' if d == 0 else str(d) + ' lines differ'}  ({len(asm[len(pairs) + k])} lines)")
        if n in a.kernels:
            ka, kb = kernel_bodies(asm[k]), kernel_bodies(asm[len(pairs) + k])
            for sym in sorted(set(ka) | set(kb)):
                what = ("only in the parent tree" if sym not in kb else "only in this tree" if sym not in ka
                        else "identical" if ka[sym] == kb[sym] else "differs")
                print(f"    {sym:60s} {what}  ({len(kb.get(sym, ka.get(sym)))} lines)")
    old_parts = {o: moved_parts(s) for o, s in asm_old.items()}
    new_parts = {n: moved_parts(s) for n, s in asm_new.items()}
    for o in sorted(moved):
        old = old_parts[o]
        print(f"{o} -> {', '.join(moved[o])}  (moved: function by function)")
        for sym in sorted(old):
            at = [n for n in moved[o] if sym in new_parts[n]]
            if len(at) != 1:
                worst = max(worst, 1)
                print(f"    {sym:60s} {'in no new file' if not at else 'in ' + ' and '.join(at)}")
                continue
            d = sum(differing_lines(x, y) for x, y in zip(old[sym], new_parts[at[0]][sym]))
            worst = max(worst, d)
            print(f"    {sym:60s} {'identical' if d == 0 else 'differs (' + str(d) + ' lines)'}  "
                  f"({len(old[sym][0])} + {len(old[sym][1])} lines, {at[0]})")
    for n in sorted(moved_new):   # what a NEW file holds beside the functions of the OLD files that name it
        known = set().union(*(old_parts[o] for o in moved if n in moved[o]))
        for sym in sorted(set(new_parts[n]) - known):
            print(f"{n:44s} {sym} only in this tree")
    for f in fa:
        if f not in paired_a:
            print(f"{f:44s} only in the parent tree")
    for f in fb:
        if f not in paired_b:
            print(f"{f:44s} only in this tree")
    return 0 if worst == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
