#!/usr/bin/env python3
"""Register and code-size account of the frame kernels, from the compiler alone (no GPU).

Compiles gv_binning.hip, gv_raysector.hip and gv_gridpass.hip device-only for gfx950 with exactly gvamd/build.py's FLAGS plus
-Rpass-analysis=kernel-resource-usage into a scratch directory and prints, per kernel instantiation: VGPRs, waves
per SIMD, spilled SGPRs / VGPRs, scratch bytes, code bytes and the static counts of VALU instructions, lane moves
(v_readlane_b32 + v_writelane_b32: a spilled scalar register lives in a lane of a vector register, and every spill
and reload is a VALU-class instruction) and s_nop.

    python3 tools/kernel_resources.py [--out DIR] [--keep] [--label TEXT] [--csrc DIR]

All counts are static; the dynamic share is a counter run's business (tools/pmc_pass.sh)."""
from __future__ import annotations

import argparse
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

FILES = ["gv_binning.hip", "gv_raysector.hip", "gv_gridpass.hip"]
REMARK = "-Rpass-analysis=kernel-resource-usage"
_FIELDS = {
    "TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs",
    "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves",
    "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds",
}


def llvm_tool(name: str) -> str:
    cc = os.path.realpath(gvbuild.hipcc())
    for d in (os.path.join(os.path.dirname(os.path.dirname(cc)), "llvm", "bin"), os.path.dirname(cc),
              "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if p:
        return p
    raise RuntimeError(name + " not found next to hipcc")


def parse_remarks(text: str) -> dict:
    """{mangled kernel name: {field: int}} from the compiler's kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
            continue
        if cur is None or ":" not in body:
            continue
        key, val = body.rsplit(":", 1)
        key, val = key.strip(), val.strip()
        if key in _FIELDS and re.fullmatch(r"-?\d+", val):
            cur[_FIELDS[key]] = int(val)
    return out


def compile_file(src: str, out_dir: str, csrc: str = gvbuild.CSRC) -> tuple:
    """Device-only compile of one csrc file; returns (code object path, remarks text)."""
    co = os.path.join(out_dir, src + ".co")
    cmd = [gvbuild.hipcc(), *gvbuild.FLAGS, REMARK, "--offload-device-only", "--no-gpu-bundle-output", "-c", "-o", co,
           os.path.join(csrc, src)]
    r = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise RuntimeError("compile failed: " + src)
    with open(os.path.join(out_dir, src + ".remarks"), "w") as f:
        f.write(r.stderr)
    return co, r.stderr


def code_sizes(co: str) -> dict:
    txt = subprocess.check_output([llvm_tool("llvm-readelf"), "-sW", co], text=True)
    sizes = {}
    for line in txt.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            sizes[p[7]] = int(p[2])
    return sizes


def static_counts(co: str, sizes: dict) -> dict:
    """{symbol: {valu, lane_moves, s_nop, insts}} from the disassembly, inside the symbol's own bytes (the padding
    between kernels disassembles as s_nop too)."""
    txt = subprocess.check_output([llvm_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, cur, end = {}, None, 0
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(2), {"valu": 0, "lane_moves": 0, "s_nop": 0, "insts": 0})
            end = int(m.group(1), 16) + sizes.get(m.group(2), 1 << 62)
            continue
        if cur is None:
            continue
        m = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if m and int(m.group(1), 16) >= end:
            continue
        t = line.split()
        if not t:
            continue
        op = t[0]
        if not re.match(r"^[a-z_]+[a-z0-9_]*$", op):
            continue
        cur["insts"] += 1
        if op.startswith("v_"):
            cur["valu"] += 1
            if op in ("v_readlane_b32", "v_writelane_b32"):
                cur["lane_moves"] += 1
        elif op == "s_nop":
            cur["s_nop"] += 1
    return out


def short_name(sym: str) -> str:
    """k_bin_partition<true,true,false> from _ZN2gv15k_bin_partitionILb1ELb1ELb0EEEvNS_7BinArgsE: the kernels here are
    gv:: functions whose template arguments are bools and ints, so no demangler is needed"""
    m = re.match(r"^_ZN2gv(\d+)", sym)
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while True:
        m = re.match(r"L([bi])(n?\d+)E", rest)
        if not m:
            break
        kind, val = m.groups()
        args.append(("true" if val == "1" else "false") if kind == "b" else val.replace("n", "-"))
        rest = rest[m.end():]
    return name + "<" + ",".join(args) + ">"


def collect(out_dir: str, csrc: str = gvbuild.CSRC) -> list:
    """One row (dict) per kernel instantiation of FILES (csrc: another checkout's csrc directory, for a comparison)."""
    with ThreadPoolExecutor(max_workers=len(FILES)) as ex:
        built = list(ex.map(lambda s: compile_file(s, out_dir, csrc), FILES))
    rows = []
    for src, (co, remarks) in zip(FILES, built):
        res, sizes = parse_remarks(remarks), code_sizes(co)
        counts = static_counts(co, sizes)
        for sym, r in res.items():
            if "waves" not in r:      # a device function, not a kernel
                continue
            row = dict(r)
            row.update(counts.get(sym, {}))
            row["file"], row["symbol"], row["kernel"] = src, sym, short_name(sym)
            row["code"] = sizes.get(sym, 0)
            rows.append(row)
    return rows


def render(rows: list) -> str:
    hdr = ("kernel", "VGPRs", "waves/SIMD", "SGPR spill", "VGPR spill", "scratch B", "code B", "VALU", "lane moves",
           "s_nop")
    keys = ("kernel", "vgprs", "waves", "sgpr_spill", "vgpr_spill", "scratch", "code", "valu", "lane_moves", "s_nop")
    table = [hdr] + [tuple(str(r.get(k, "?")) for k in keys) for r in rows]
    wid = [max(len(t[i]) for t in table) for i in range(len(hdr))]
    lines = []
    for t in table:
        lines.append("  ".join(t[i].ljust(wid[i]) if i == 0 else t[i].rjust(wid[i]) for i in range(len(hdr))))
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="scratch directory (default: a temporary one)")
    ap.add_argument("--keep", action="store_true", help="keep the scratch directory (code objects, remarks)")
    ap.add_argument("--label", default="", help="heading printed above the table")
    ap.add_argument("--csrc", default=gvbuild.CSRC, help="compile FILES of another csrc directory (a parent checkout)")
    a = ap.parse_args()
    out_dir = a.out or tempfile.mkdtemp(prefix="gv_kres_")
    os.makedirs(out_dir, exist_ok=True)
    try:
        rows = collect(out_dir, os.path.abspath(a.csrc))
    finally:
        if not (a.keep or a.out):
            shutil.rmtree(out_dir, ignore_errors=True)
    if a.label:
        print("== " + a.label)
    print("flags: " + " ".join(gvbuild.FLAGS))
    print(render(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
