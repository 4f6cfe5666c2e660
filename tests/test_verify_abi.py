"""CPU: the verify / scrub entry points are declared the same way on every
side of the boundary -- header, linker map, Rust crate, ctypes mirror -- the
Python constants equal the header's, and the scrub's states -> verdict logic
(maxio_amd/csrc/scrub_plan.hpp) does what mxec_scrub_object documents, run
as a stand-alone program under -fsanitize=address,undefined.  No kernel is
launched here.

Replaces: the crate's ReedSolomon::verify (reed-solomon-erasure 6.0.0) and a
scrubber MaxIO does not have."""
from __future__ import annotations

import ctypes
import fnmatch
import os
import re
import shutil
import subprocess

import pytest

import maxio_amd
from maxio_amd import _native, ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxio_ec.h")
NEW = ["mxec_verify", "mxec_verify_strided_device", "mxec_verify_batch_device", "mxec_scrub_object"]
ARITY = {"mxec_verify": 9, "mxec_verify_strided_device": 15, "mxec_verify_batch_device": 9, "mxec_scrub_object": 4}


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_new_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    p = _header_params("mxec_verify")
    assert p[3].startswith("size_t ") and p[6].startswith("const uint8_t* const*") and p[7].startswith("uint64_t*")
    p = _header_params("mxec_verify_strided_device")
    assert p[7].startswith("const uint8_t*") and p[11].startswith("const uint8_t*") and p[14].startswith("uint64_t*")
    assert "#define MXEC_VERIFY_OK UINT64_MAX" in open(HEADER).read()


def test_map_exports_them():
    text = open(os.path.join(ROOT, "maxio_amd", "csrc", "maxio_ec.map")).read()
    glob = re.search(r"global:\s*([^;]+);", text).group(1).split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name
    if os.path.exists(maxio_amd.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", maxio_amd.LIB_PATH], capture_output=True, text=True,
                             check=True).stdout
        for name in NEW:
            assert re.search(r"\bT %s$" % name, out, re.M), name


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "rust", "maxio-ec-sys", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    for name in NEW:
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, block, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == ARITY[name], name
    assert "pub const MXEC_VERIFY_OK: u64 = u64::MAX;" in src
    # the report struct, field for field (the header keeps it out of the
    # typedef-struct form tests/test_rust_ffi.py enumerates)
    body = re.search(r"pub struct MxecScrubReport \{(.*?)\}", src, flags=re.S).group(1)
    fields = [tuple(x.strip() for x in f.replace("pub ", "").split(":")) for f in body.split(",") if f.strip()]
    assert fields == [("k", "u32"), ("m", "u32"), ("verdict", "u32"), ("n_damaged", "u32"), ("n_healed", "u32"),
                      ("parity_consistent", "i32"), ("parity_first_bad", "u64"), ("shard_state", "[u8; 256]")]


def test_ctypes_mirror_binds_them_with_matching_arity():
    for name in NEW:
        res, args = _native._SIGS[name]
        assert res is _native.INT and len(args) == ARITY[name], name
    assert hasattr(maxio_amd.lib(), "mxec_scrub_object")
    for meth in ("verify", "verify_strided_device", "verify_batch_device", "scrub_object"):
        assert callable(getattr(maxio_amd.Context, meth))


def test_report_struct_layout_matches_the_header(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct mxec_scrub_report \{(.*?)\};", text, flags=re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t k, m, verdict, n_damaged, n_healed", "int32_t parity_consistent",
                     "uint64_t parity_first_bad", "uint8_t shard_state[256]"]
    R = _native.ScrubReport
    assert [f[0] for f in R._fields_] == ["k", "m", "verdict", "n_damaged", "n_healed", "parity_consistent",
                                          "parity_first_bad", "shard_state"]
    assert (R.parity_consistent.offset, R.parity_first_bad.offset, R.shard_state.offset) == (20, 24, 32)
    assert ctypes.sizeof(R) == 32 + 256
    if shutil.which("gcc"):  # the C compiler's own layout
        src = tmp_path / "t.c"
        src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "maxio_ec.h"\nint main(void){ mxec_scrub_report r; '
                       'printf("%zu %zu %zu %zu\\n", sizeof r, offsetof(mxec_scrub_report, parity_consistent), '
                       'offsetof(mxec_scrub_report, parity_first_bad), offsetof(mxec_scrub_report, shard_state)); '
                       'return MXEC_VERIFY_OK == UINT64_MAX ? 0 : 1; }\n')
        exe = tmp_path / "t"
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
        assert [int(x) for x in out] == [288, 20, 24, 32]


def test_python_constants_equal_the_headers():
    defs = {n: int(v, 0) for n, v in
            re.findall(r"#define\s+(MXEC_(?:SCRUB|SHARD)_\w+)\s+((?:0x)?[0-9a-fA-F]+)u?\b", open(HEADER).read())}
    assert len(defs) == 12
    for name, val in defs.items():
        assert getattr(ec, name[len("MXEC_"):]) == val, name
    assert defs["MXEC_SCRUB_PARITY"] == 1 and defs["MXEC_SCRUB_DIGESTS"] == 2 and defs["MXEC_SCRUB_HEAL"] == 4
    assert [defs["MXEC_SCRUB_" + n] for n in ("CLEAN", "DAMAGED", "HEALED", "UNRECOVERABLE")] == [0, 1, 2, 3]
    assert [defs["MXEC_SHARD_" + n] for n in ("OK", "MISSING", "BAD_SIZE", "BAD_DIGEST", "HEALED")] == [0, 1, 2, 3, 0x80]
    assert ec.VERIFY_OK == 2 ** 64 - 1


# ---- states -> verdict, stand-alone under the sanitizers -----------------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
CLEAN, DAMAGED, HEALED, UNRECOVERABLE = 0, 1, 2, 3

# (m, heal, parity_consistent, rebuilt_ok, states) -> (n_damaged, can_heal, verdict)
CASES = [
    ((2, 0, 1, 0, [0] * 6), (0, 0, CLEAN)),
    ((2, 0, -1, 0, [0] * 6), (0, 0, CLEAN)),
    ((2, 1, 1, 0, [0] * 6), (0, 0, CLEAN)),                       # heal asked, nothing to do
    ((2, 0, 0, 0, [0] * 6), (0, 0, DAMAGED)),                     # parity mismatch, no shard named
    ((2, 1, 0, 0, [0] * 6), (0, 0, DAMAGED)),                     # ... and nothing a heal could rebuild
    ((2, 0, -1, 0, [0, 1, 0, 0, 0, 0]), (1, 1, DAMAGED)),         # not asked to heal
    ((2, 1, -1, 1, [0, 1, 0, 0, 0, 2]), (2, 1, HEALED)),
    ((2, 1, -1, 0, [0, 1, 0, 0, 0, 2]), (2, 1, UNRECOVERABLE)),   # a rebuilt digest disagreed
    ((2, 1, -1, 0, [3, 1, 0, 0, 0, 2]), (3, 0, UNRECOVERABLE)),   # more than m
    ((2, 1, -1, 1, [3, 1, 0, 0, 0, 2]), (3, 0, UNRECOVERABLE)),   # never HEALED past m
    ((0, 1, -1, 0, [0, 3, 0]), (1, 0, UNRECOVERABLE)),            # no parity: nothing to rebuild from
    ((0, 0, -1, 0, [0, 3, 0]), (1, 0, DAMAGED)),
    ((2, 0, -1, 0, [0x81, 0x82, 0, 0, 0, 0]), (2, 1, DAMAGED)),   # the HEALED bit keeps the finding
    ((1, 1, -1, 1, [0] * 255 + [1]), (1, 1, HEALED)),             # the report's last entry
    ((4, 1, -1, 1, []), (0, 0, CLEAN)),
]


def test_states_to_verdict_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "scrub_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", "scrub_plan_check.cpp")], check=True)
    text = "".join("%d %d %d %d %s\n" % (m, heal, pc, ok, " ".join(map(str, st))) for (m, heal, pc, ok, st), _ in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert got == [want for _, want in CASES]
