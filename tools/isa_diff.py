#!/usr/bin/env python3
"""Whether two versions of a HIP kernel file compile to the same gfx950 code.

  python tools/isa_diff.py OLD.hip NEW.hip
  python tools/isa_diff.py --rev HEAD~1 [--rev2 REV] maxio_amd/csrc/rs_kernel.hip

--rev takes the old side from that git revision (with its directory, for the
headers); the new side is the working tree, or --rev2.  Per new kernel: the
old kernels of the same base name whose instruction stream (symbol names and
block-label numbers normalised) and register / LDS / scratch sizes are equal,
else a unified diff against the closest-named one; then the old kernels that
nothing matched.  Text comparison only.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_count import ROOT, assemble  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(lines: list[str]) -> dict[str, tuple[list[str], tuple]]:
    """Demangled kernel name -> (normalised instructions and labels, META values)."""
    meta: dict[str, dict[str, str]] = {}
    for entry in re.split(r"^  - ", "\n".join(lines).split("amdhsa.kernels:")[-1], flags=re.M)[1:]:
        f = dict(re.findall(r"^ {0,4}(\.\w+): +(\S+)$", entry, re.M))
        if ".name" in f:  # the version list's entries split off too
            meta[f[".name"]] = f
    body = {name: [] for name in meta}
    cur = None
    for ln in lines:
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in body:
            cur = body[m.group(1)]
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and (ln.startswith(".LBB") or re.match(r"^\t[a-z]", ln)):
            ln = re.sub(r"\s*;.*", "", ln)
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", ln)))
    names = subprocess.run(["c++filt"], input="\n".join(body), capture_output=True, text=True, check=True).stdout
    short = [re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", ""))
             for n in names.splitlines()]
    return {s: (body[n], tuple(meta[n][k] for k in META)) for s, n in zip(short, body)}


def at_rev(rev: str, path: str, tmp: str) -> str:
    rel = os.path.relpath(os.path.abspath(path), ROOT)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, os.path.dirname(rel)], capture_output=True, check=True)
    subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
    return os.path.join(tmp, rel)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src", nargs="+", help="OLD NEW, or one file with --rev")
    ap.add_argument("--rev", help="old side: the file at this git revision")
    ap.add_argument("--rev2", help="new side: at this revision (default: the working tree)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        old = kernels(assemble(at_rev(a.rev, a.src[0], t1) if a.rev else a.src[0]))
        new = kernels(assemble(at_rev(a.rev2, a.src[-1], t2) if a.rev2 else a.src[-1]))
    used, differ = set(), 0
    for n, (ins, meta) in sorted(new.items()):
        peers = [o for o in old if o.split("<")[0] == n.split("<")[0]]
        same = [o for o in peers if old[o] == (ins, meta)]
        used.update(same)
        if same:
            print(f"same  {n}  ==  {', '.join(same)}  "
                  f"[{sum(not x.startswith('.') for x in ins)} instructions, {dict(zip(META, meta))}]")
            continue
        differ += 1
        near = difflib.get_close_matches(n, peers, 1, 0.0)
        if not near:
            print(f"NEW   {n}  (no old kernel of this name)")
            continue
        o_ins, o_meta = old[near[0]]
        print(f"DIFF  {n}  vs  {near[0]}  meta {dict(zip(META, o_meta))} -> {dict(zip(META, meta))}")
        sys.stdout.writelines(x + "\n" for x in difflib.unified_diff(o_ins, ins, near[0], n, lineterm="", n=2))
    gone = sorted(set(old) - used)
    print("".join(f"gone  {o}\n" for o in gone), end="")
    print(f"{len(old)} old kernels, {len(new)} new: {len(new) - differ} identical, {differ} differ or new, "
          f"{len(gone)} old ones unmatched")
    return 1 if differ else 0


if __name__ == "__main__":
    raise SystemExit(main())
