"""CPU: the locate entry points (mxec_locate, mxec_locate_strided_device,
mxec_locate_batch_device, mxec_locate_outcome, mxec_locate_object) are
declared the same way on every side of the boundary -- header, linker map,
Rust crate, ctypes mirror --, both structs have one layout everywhere, the
Python constants equal the header's, mxec_locate_outcome's truth table holds,
and the host builder of the per-(k, m) ratio -> shard table
(maxio_amd/csrc/locate_plan.hpp) gives what the restatement over the oracle's
matrix gives (tests/locate_ref.py), run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Reference: none -- the crate has no locator and MaxIO no scrubber (SURVEY.md
§3.2, §5); the algebra is restated in tests/locate_ref.py."""
from __future__ import annotations

import ctypes
import fnmatch
import os
import re
import shutil
import subprocess

import pytest

import locate_ref
import maxio_amd
import oracle
from maxio_amd import _native, ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxio_ec.h")
NEW = ["mxec_locate", "mxec_locate_strided_device", "mxec_locate_batch_device", "mxec_locate_outcome",
       "mxec_locate_object"]
ARITY = {"mxec_locate": 8, "mxec_locate_strided_device": 15, "mxec_locate_batch_device": 9,
         "mxec_locate_outcome": 2, "mxec_locate_object": 4}


def _header_text() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_params(name: str) -> list[str]:
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, _header_text(), flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_five_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    # the verify calls' argument shapes, the result pointer in first_bad's place
    for loc, ver in (("mxec_locate", "mxec_verify"), ("mxec_locate_strided_device", "mxec_verify_strided_device"),
                     ("mxec_locate_batch_device", "mxec_verify_batch_device")):
        a, b = _header_params(loc), _header_params(ver)
        n = ARITY[loc] - 1
        assert [p.rsplit(" ", 1)[0] for p in a[:n]] == [p.rsplit(" ", 1)[0] for p in b[:n]], loc
        assert a[n].startswith("void*"), loc
    assert "#define MXEC_LOCATE_NO_SHARD 0xFFFFFFFEu" in open(HEADER).read()


def test_map_exports_them():
    text = open(os.path.join(ROOT, "maxio_amd", "csrc", "maxio_ec.map")).read()
    glob = re.search(r"global:\s*([^;]+);", text).group(1).split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name
    assert os.path.exists(maxio_amd.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", maxio_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s$" % name, out, re.M), name


RUST_RESULT = [("first_bad", "u64"), ("n_bad", "u64"), ("shard_min", "u32"), ("shard_max", "u32")]
RUST_REPORT = [("k", "u32"), ("m", "u32"), ("outcome", "u32"), ("shard", "u32"), ("first_bad", "u64"), ("n_bad", "u64"),
               ("healed", "u32"), ("reserved", "u32")]


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "rust", "maxio-ec-sys", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    for name in NEW:
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, block, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == ARITY[name], name
    for struct, want in (("MxecLocateResult", RUST_RESULT), ("MxecLocateReport", RUST_REPORT)):
        body = re.search(r"#\[repr\(C\)\][^\n]*\n(?:#\[[^\n]*\]\n)*pub struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
        fields = [tuple(x.strip() for x in f.replace("pub ", "").split(":")) for f in body.split(",") if f.strip()]
        assert fields == want, struct
    for name, val in _header_constants().items():
        assert re.search(r"pub const %s: u32 = (0x[0-9A-Fa-f]+|\d+);" % name, src), name
        got = int(re.search(r"pub const %s: u32 = (0x[0-9A-Fa-f]+|\d+);" % name, src).group(1), 0)
        assert got == val, name


def test_ctypes_mirror_binds_them_with_matching_arity():
    for name in NEW:
        res, args = _native._SIGS[name]
        assert res is _native.INT and len(args) == ARITY[name], name
        assert hasattr(maxio_amd.lib(), name)
    for meth in ("locate", "locate_strided_device", "locate_batch_device", "locate_object"):
        assert callable(getattr(maxio_amd.Context, meth))
    assert callable(maxio_amd.ReedSolomon.locate)


def _struct_decls(name: str) -> list[str]:
    body = re.search(r"struct %s \{(.*?)\};" % name, _header_text(), flags=re.S).group(1)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


def test_struct_layouts_match_the_header(tmp_path):
    assert _struct_decls("mxec_locate_result") == ["uint64_t first_bad", "uint64_t n_bad", "uint32_t shard_min",
                                                   "uint32_t shard_max"]
    assert _struct_decls("mxec_locate_report") == ["uint32_t k, m, outcome, shard", "uint64_t first_bad, n_bad",
                                                   "uint32_t healed, reserved"]
    R, P = _native.LocateResult, _native.LocateReport
    assert [f[0] for f in R._fields_] == ["first_bad", "n_bad", "shard_min", "shard_max"]
    assert [f[0] for f in P._fields_] == ["k", "m", "outcome", "shard", "first_bad", "n_bad", "healed", "reserved"]
    py = [ctypes.sizeof(R), R.first_bad.offset, R.n_bad.offset, R.shard_min.offset, R.shard_max.offset,
          ctypes.sizeof(P), P.k.offset, P.m.offset, P.outcome.offset, P.shard.offset, P.first_bad.offset,
          P.n_bad.offset, P.healed.offset, P.reserved.offset]
    assert py == [24, 0, 8, 16, 20, 40, 0, 4, 8, 12, 16, 24, 32, 36]
    assert ec.LOCATE_RESULT_BYTES == 24
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    fields_r = ["first_bad", "n_bad", "shard_min", "shard_max"]
    fields_p = ["k", "m", "outcome", "shard", "first_bad", "n_bad", "healed", "reserved"]
    prints = ['printf("%zu\\n", sizeof(mxec_locate_result));']
    prints += ['printf("%%zu\\n", offsetof(mxec_locate_result, %s));' % f for f in fields_r]
    prints += ['printf("%zu\\n", sizeof(mxec_locate_report));']
    prints += ['printf("%%zu\\n", offsetof(mxec_locate_report, %s));' % f for f in fields_p]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "maxio_ec.h"\nint main(void){ %s return 0; }\n'
                   % " ".join(prints))
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == py


def _header_constants() -> dict:
    return {n: int(v, 0) for n, v in
            re.findall(r"#define\s+(MXEC_LOCATE_\w+)\s+((?:0x)?[0-9a-fA-F]+)u?\b", open(HEADER).read())}


def test_python_constants_equal_the_headers():
    defs = _header_constants()
    assert sorted(defs) == ["MXEC_LOCATE_CLEAN", "MXEC_LOCATE_F_HEAL", "MXEC_LOCATE_MANY", "MXEC_LOCATE_NO_SHARD",
                            "MXEC_LOCATE_ONE", "MXEC_LOCATE_SKIPPED"]
    for name, val in defs.items():
        assert getattr(ec, name[len("MXEC_"):]) == val, name
        assert getattr(maxio_amd, name[len("MXEC_"):]) == val, name
    assert [defs["MXEC_LOCATE_" + n] for n in ("CLEAN", "ONE", "MANY", "SKIPPED")] == [0, 1, 2, 3]
    assert defs["MXEC_LOCATE_NO_SHARD"] == 0xFFFFFFFE == locate_ref.NO_SHARD and defs["MXEC_LOCATE_F_HEAL"] == 1


# (first_bad, n_bad, shard_min, shard_max) -> (outcome, shard)
NO = 0xFFFFFFFE
OUTCOMES = [
    ((locate_ref.OK, 0, 0xFFFFFFFF, 0), (ec.LOCATE_CLEAN, None)),     # clean
    ((17, 1, 3, 3), (ec.LOCATE_ONE, 3)),                              # one shard
    ((0, 90000, 0, 0), (ec.LOCATE_ONE, 0)),
    ((5, 2, 5, 255), (ec.LOCATE_MANY, None)),
    ((9, 4, 255, 255), (ec.LOCATE_ONE, 255)),                         # the last index a stripe can have
    ((5, 2, 1, 4), (ec.LOCATE_MANY, None)),                           # two different shards
    ((5, 7, NO, NO), (ec.LOCATE_MANY, None)),                         # NO_SHARD only
    ((5, 7, 2, NO), (ec.LOCATE_MANY, None)),                          # one shard plus NO_SHARD
    ((5, 1, 256, 256), (ec.LOCATE_MANY, None)),                       # shard_min == shard_max >= 256
    ((5, 1, 0xFFFFFFFF, 0xFFFFFFFF), (ec.LOCATE_MANY, None)),
]


def test_outcome_truth_table_through_ctypes():
    lib = maxio_amd.lib()
    for rec, want in OUTCOMES:
        r = _native.LocateResult(*rec)
        shard = ctypes.c_uint32(0xDEAD)
        got = lib.mxec_locate_outcome(ctypes.byref(r), ctypes.byref(shard))
        assert (got, shard.value if got == ec.LOCATE_ONE else None) == want, rec
        if got != ec.LOCATE_ONE:
            assert shard.value == 0xDEAD, rec  # written only when it means something
        assert lib.mxec_locate_outcome(ctypes.byref(r), None) == want[0], rec  # shard may be NULL
        assert ec.locate_outcome(*rec) == want == locate_ref.outcome(rec), rec


# ---- the ratio -> shard table, stand-alone under the sanitizers ----------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("locate_plan") / "locate_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", "locate_plan_check.cpp")], check=True)

    def run(lines: list[str]) -> list[list[int]]:
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=ENV,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run


def _error_codes():
    defs = dict(re.findall(r"#define\s+(MXEC_E_\w+)\s+\(?(-?\d+)\)?", open(HEADER).read()))
    return int(defs["MXEC_E_SINGULAR_MATRIX"]), int(defs["MXEC_E_INVALID_ARG"])


def _log_ratio(a: int, b: int) -> int:
    """log2 of a / b in the field, by counting multiplications by 2."""
    want, x, n = oracle.gf_div(a, b), 1, 0
    while x != want:
        x, n = oracle.gf_mul(x, 2), n + 1
    return n


def _raw(k: int, m: int, rows) -> str:
    return "raw %d %d " % (k, m) + " ".join(str(int(x)) for x in rows.reshape(-1))


def test_ratio_table_equals_the_restatement(plan_check):
    """The builder over the library's own parity rows (mxec_rs_parity_matrix,
    what ops.cpp hands it) against the restatement over the oracle's."""
    shapes = [(k, 2) for k in range(1, 254)] + [(4, 2), (8, 4), (10, 4), (6, 8)]
    got = plan_check([_raw(k, m, maxio_amd.parity_matrix(k, m)) for (k, m) in shapes])
    for (k, m), row in zip(shapes, got):
        assert row[0] == 0, (k, m)
        assert row[1:257] == locate_ref.ratio_table(k, m), (k, m)  # asserts no collision on its side
        assert sorted(x for x in row[1:257] if x != 0xFF) == list(range(k)), (k, m)
    # the rows the kernel confirms a candidate against: log(M[i][j] / M[0][j])
    for (k, m), row in zip(shapes[-3:], got[-3:]):
        M = locate_ref.parity_rows(k, m)
        want = [0 if i == 0 else _log_ratio(int(M[i, j]), int(M[0, j])) for i in range(m) for j in range(k)]
        assert row[257:] == want, (k, m)


def test_ratio_table_builder_rejects_what_is_not_mds(plan_check):
    singular, invalid = _error_codes()
    M =locate_ref.parity_rows(4, 2)
    prop = M.copy()
    prop[:, 3] = [oracle.gf_mul(int(x), 7) for x in prop[:, 1]]  # column 3 = 7 * column 1
    zero = M.copy()
    zero[1, 2] = 0
    lines = [_raw(4, 2, M), _raw(4, 2, prop), _raw(4, 2, zero), _raw(4, 1, M[:1]),
             _raw(4, 9, locate_ref.parity_rows(4, 9)), "raw 0 2", "raw 255 2 " + " ".join(["1"] * 510)]
    got = plan_check(lines)
    assert got[0][0] == 0 and got[0][1:257] == locate_ref.ratio_table(4, 2)
    assert [g[0] for g in got[1:]] == [singular, singular, invalid, invalid, invalid, invalid]


def test_outcome_logic_stand_alone(plan_check):
    got = plan_check(["out %d %d %d %d" % rec for rec, _ in OUTCOMES])
    for (rec, (want, shard)), (o, s) in zip(OUTCOMES, got):
        assert o == want and (s == shard if want == ec.LOCATE_ONE else s == 0xDEAD), rec
