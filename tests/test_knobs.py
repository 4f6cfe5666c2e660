"""CPU: the shipping library's configuration surface.

* The MXEC_* names inside libmaxio_ec.so (the strings its getenv calls use)
  are exactly the ones INTEGRATION.md §3's product and test-only tables
  document, and the lab build's extra names are the lab list.
* The shipping library instantiates exactly the kernel geometries a launch
  can reach, and a lab build the same ones.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "maxio_amd", "lib", "libmaxio_ec.so")
LAB = os.path.join(ROOT, "maxio_amd", "lib", "libmaxio_ec_lab.so")
DOC = os.path.join(ROOT, "INTEGRATION.md")


def _names_in(path):
    with open(path, "rb") as f:
        return {m.decode() for m in re.findall(rb"MXEC_[A-Z0-9_]+", f.read())}


def _doc_tables():
    text = open(DOC).read()
    sec = text[text.index("Environment knobs"):text.index("## 4. Device-resident callers")]
    tables, lab = sec.split("Lab build only")
    documented = set(re.findall(r"^\| `(MXEC_[A-Z0-9_]+)`", tables, re.M))
    lab_names = set(re.findall(r"`(MXEC_[A-Z0-9_]+)", lab))
    return documented, lab_names


def test_product_library_reads_exactly_the_documented_knobs():
    if not os.path.exists(LIB):
        pytest.skip("libmaxio_ec.so not built")
    documented, _ = _doc_tables()
    assert _names_in(LIB) == documented


def test_lab_build_adds_only_the_documented_lab_knobs():
    if not os.path.exists(LAB):
        pytest.skip("lab build not present (make -C maxio_amd/csrc lab)")
    documented, lab = _doc_tables()
    extra = _names_in(LAB) - _names_in(LIB)
    assert extra <= lab - {"MXEC_LIB"}, extra - lab
    assert _names_in(LAB) >= _names_in(LIB)


def _kernels(path):
    """The library's rs_*_fast and sha256_ kernels, as 'name<args>' without
    namespaces (the fat binary's symbols: one local data symbol per kernel)."""
    out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    names = [re.sub(r"\(.*", "", ln.split(" ", 2)[2].replace("(anonymous namespace)", "anon"))
             for ln in out.splitlines()
             if " d " in ln and ("_fast<" in ln or "sha256_" in ln) and ".kd" not in ln]
    return sorted(n.replace("void ", "").split("::")[-1] for n in names)


def _fast_set(family, uniform_v2, r_min=1):
    """R = r_min..8, uniform and grouped, at V = 4 for R <= 4 and 2 beyond;
    uniform_v2: also the uniform R <= 4 kernels at V = 2, which the last row
    block of a launch of 9..12 rows in all runs (the launch's tile size is
    its total row count's)."""
    want = [f"{family}<{r}, {4 if r <= 4 else 2}, {grp}>" for r in range(r_min, 9) for grp in ("false", "true")]
    if uniform_v2:
        want += [f"{family}<{r}, 2, false>" for r in range(r_min, 5)]
    return sorted(want)


def test_product_library_has_only_default_kernel_instantiations():
    """Exactly the kernels a launch can reach; a lab build, where present,
    holds the same ones (its knobs change launch parameters only)."""
    if not os.path.exists(LIB):
        pytest.skip("libmaxio_ec.so not built")
    ks = _kernels(LIB)
    if os.path.exists(LAB):
        assert _kernels(LAB) == ks
    assert [k for k in ks if k.startswith("rs_apply_fast<")] == _fast_set("rs_apply_fast", True)
    assert [k for k in ks if k.startswith("rs_verify_fast<")] == _fast_set("rs_verify_fast", True)
    assert [k for k in ks if k.startswith("rs_locate_fast<")] == _fast_set("rs_locate_fast", False, r_min=2)
    assert [k for k in ks if k.startswith("sha256_")] == [
        "sha256_kernel", "sha256_quad_kernel", "sha256_split_kernel", "sha256_stream_kernel"]


def test_entry_point_count_matches_the_docs():
    """DESIGN.md and INTEGRATION.md state how many functions the header
    declares (the counts had drifted apart)."""
    hdr = open(os.path.join(ROOT, "include", "maxio_ec.h")).read()
    n = len(set(re.findall(r"\b(mxec_[a-z_0-9]+)\s*\(", hdr)))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    integ = open(DOC).read()
    assert f"{n} entry points" in design and f"{n} functions" in design, n
    assert f"header's {n} functions" in integ, n
