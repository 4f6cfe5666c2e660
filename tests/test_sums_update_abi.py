"""CPU: the resumable body digests' entry points -- mxec_body_sums_update_device,
mxec_writer_open_sums, mxec_writer_sums -- and their three constants are
declared the same way on every side of the boundary (header, linker map, Rust
crate, ctypes mirror, Python classes); the state record fits the caller's
MXEC_SUMS_STATE_BYTES; and the two pieces of arithmetic behind them
(maxio_amd/csrc/sums_carry.hpp, the digest runs of writer_plan.hpp) do what
they document, each run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Replaces: Md5::update / ChecksumHasher::update per stream piece
(filesystem.rs:722-725) and PutResult's etag / checksum_value (:775-777)."""
from __future__ import annotations

import fnmatch
import os
import re
import shutil
import subprocess

import pytest

import maxio_amd
from maxio_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxio_ec.h")
CSRC = os.path.join(ROOT, "maxio_amd", "csrc")
ARITY = {"mxec_body_sums_update_device": 10, "mxec_writer_open_sums": 9, "mxec_writer_sums": 2}
CONSTS = {"MXEC_SUMS_STATE_BYTES": 512, "MXEC_SUMS_F_FIRST": 1, "MXEC_SUMS_F_FINAL": 2}


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_them():
    text = open(HEADER).read()
    for name, n in ARITY.items():
        assert len(_header_params(name)) == n, name
    for name, v in CONSTS.items():
        assert re.search(r"#define\s+%s\s+%du\b" % (name, v), text), name
    p = _header_params("mxec_body_sums_update_device")
    assert p[3].startswith("const uint8_t* const*") and p[4].startswith("const uint64_t*")
    assert [x.split()[0] for x in p[5:8]] == ["uint64_t", "uint32_t", "uint32_t"]
    assert p[8] == "void* state_dev" and p[9] == "mxec_body_sums* out_dev"
    p = _header_params("mxec_writer_open_sums")
    assert _header_params("mxec_writer_open") == p[:7] + p[8:] and p[7] == "uint32_t which"
    assert _header_params("mxec_writer_sums") == ["void* w", "mxec_body_sums* out"]
    # each says what it replaces, and what a frame stream's digests are of
    upd = text[:text.index("int mxec_body_sums_update_device")][-2500:]
    assert "Md5::update" in upd and "ChecksumHasher::update" in upd and "filesystem.rs:722-725" in upd
    doc = text[text.index("mxec_writer_open_sums / mxec_writer_sums"):text.index("typedef struct mxec_writer")]
    assert "filesystem.rs:700-725" in doc and ":775-777" in doc
    assert "sums before finish" in doc and "frame stream's" in doc and "not the plaintext's" in doc


def test_map_exports_them():
    text = open(os.path.join(CSRC, "maxio_ec.map")).read()
    glob = re.search(r"global:\s*([^;]+);", text).group(1).split()
    for name in ARITY:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name
    if os.path.exists(maxio_amd.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", maxio_amd.LIB_PATH], capture_output=True, text=True,
                             check=True).stdout
        for name in ARITY:
            assert re.search(r"\bT %s$" % name, out, re.M), name


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "rust", "maxio-ec-sys", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    for name, n in ARITY.items():
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, block, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == n, name
    for name, v in CONSTS.items():
        assert re.search(r"pub const %s: u32 = %d;" % (name, v), src), name


def test_ctypes_mirror_and_python_classes():
    import inspect

    for name, n in ARITY.items():
        res, args = _native._SIGS[name]
        assert len(args) == n and res is _native.INT, name
        assert hasattr(maxio_amd.lib(), name)
    assert (maxio_amd.SUMS_STATE_BYTES, maxio_amd.SUMS_F_FIRST, maxio_amd.SUMS_F_FINAL) == (512, 1, 2)
    for c in ("SUMS_STATE_BYTES", "SUMS_F_FIRST", "SUMS_F_FINAL"):
        assert c in maxio_amd.__all__
    sig = inspect.signature(maxio_amd.Context.body_sums_update_device)
    assert list(sig.parameters)[1:] == ["ptrs", "lens", "state_ptr", "out_ptr", "which", "flags", "dev", "stream"]
    sig = inspect.signature(maxio_amd.Context.open_writer)
    assert sig.parameters["which"].default == 0
    assert callable(maxio_amd.ChunkWriter.sums)


def test_state_record_fits_the_callers_bytes(tmp_path):
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert re.search(r"static_assert\(sizeof\(SumsState\)\s*<=\s*MXEC_SUMS_STATE_BYTES", text)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "fits.hip"
    src.write_text('#include "kernels.hpp"\n'
                   "static_assert(sizeof(mxec::SumsState) % 16 == 0 && sizeof(mxec::SumsChain) % 16 == 0, \"16-byte parts\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-fsyntax-only", "-I", CSRC, str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the arithmetic, stand-alone under the sanitizers ---------------------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
U64 = 2 ** 64 - 1
MIB = 1 << 20
C2 = 2 * MIB + 20  # a chunk that crosses the run cut twice
T2 = 2 * C2 + 777
TOP = 2 ** 64 - MIB  # the last MiB mark below 2^64


def _build(tmp_path, name):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", name + ".cpp")], check=True)
    return exe


def _clean(r):
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_sums_carry_under_sanitizers(tmp_path):
    """Every pending 0..63 x len 0..200: head + 64 * blocks + rest == pending +
    len and the new tail < 64; the padding block count at 0 / 55 / 56 / 63;
    the blocks of a message cut in three are the message's."""
    exe = _build(tmp_path, "sums_carry_check")
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    _clean(r)
    assert r.stdout.splitlines() == ["identity ok %d" % (64 * 201), "pad ok 64", "replay ok %d" % 12 ** 3, "wide ok 15"]


# (case line, answer line).  Runs are at:len:first:last:closes.
RUN_CASES = [
    # nothing is due before a run's last byte is there
    ("due 100 250 0 0 40", "-"),
    ("due 100 250 0 40 100", "0:100:1:0:1"),
    ("due 100 250 1 99 100", "0:100:0:0:1"),
    ("due 100 250 2 0 50", "0:50:0:1:1"),               # the short last chunk: the body's last run
    ("due 100 100 0 0 100", "0:100:1:1:1"),             # one chunk: first and last at once
    ("due 100 0 0 0 0", "0:0:1:1:1"),                   # the empty body's one empty run
    # a chunk that crosses the 1 MiB cut
    ("due %d %d 0 0 %d" % (C2, T2, MIB - 1), "-"),
    ("due %d %d 0 0 %d" % (C2, T2, MIB), "0:%d:1:0:0" % MIB),
    ("due %d %d 0 %d %d" % (C2, T2, MIB - 1, MIB), "0:%d:1:0:0" % MIB),    # a one-byte write completes a run
    ("due %d %d 0 %d %d" % (C2, T2, MIB, MIB + 5), "-"),
    ("due %d %d 0 %d %d" % (C2, T2, MIB - 1, 2 * MIB + 1), "0:%d:1:0:0 %d:%d:0:0:0" % (MIB, MIB, MIB)),
    ("due %d %d 0 %d %d" % (C2, T2, 2 * MIB, C2), "%d:20:0:0:1" % (2 * MIB)),
    ("due %d %d 0 0 %d" % (C2, T2, C2), "0:%d:1:0:0 %d:%d:0:0:0 %d:20:0:0:1" % (MIB, MIB, MIB, 2 * MIB)),
    ("due %d %d 1 5 %d" % (C2, T2, MIB), "0:%d:0:0:0" % MIB),
    ("due %d %d 2 0 777" % (C2, T2), "0:777:0:1:1"),
    # a chunk of whole MiBs: its last run ends on a mark and closes it
    ("due %d %d 0 0 %d" % (2 * MIB, 2 * MIB, 2 * MIB), "0:%d:1:0:0 %d:%d:0:1:1" % (MIB, MIB, MIB)),
    # just below 2^64: at + 1 MiB would wrap; the chunk's end is taken instead
    ("due %d %d 0 %d %d" % (U64, U64, U64 - 5, U64), "%d:%d:0:1:1" % (TOP, MIB - 1)),
    ("due %d %d 0 %d %d" % (U64, U64, TOP - 1, TOP), "%d:%d:0:0:0" % (TOP - MIB, MIB)),
    ("due %d %d 0 %d %d" % (U64, U64, TOP - 1, U64), "%d:%d:0:0:0 %d:%d:0:1:1" % (TOP - MIB, MIB, TOP, MIB - 1)),
    ("due %d %d 0 %d %d" % (U64, U64, TOP, U64 - 1), "-"),
    # how many runs a chunk has
    ("count 100 250 0", "1"), ("count 100 0 0", "1"), ("count %d %d 0" % (C2, T2), "3"), ("count %d %d 2" % (C2, T2), "1"),
    ("count %d %d 0" % (MIB, MIB), "1"), ("count %d %d 0" % (MIB + 1, MIB + 1), "2"), ("count %d %d 0" % (U64, U64), str(2 ** 44)),
    # whole bodies in write() calls of one size: runs, firsts, lasts, chunks closed.  The program checks
    # that the runs tile every chunk exactly once, in order, on MiB marks or the chunk's end.
    ("body 100 250 7", "3 1 1 3"),
    ("body 100 250 250", "3 1 1 3"),
    ("body 100 0 1", "1 1 1 1"),
    ("body 20000 60777 1", "4 1 1 4"),
    ("body %d %d 4099" % (C2, T2), "7 1 1 3"),
    ("body %d %d %d" % (C2, T2, T2), "7 1 1 3"),
    ("body %d %d %d" % (MIB, 3 * MIB, MIB), "3 1 1 3"),
    ("body %d %d 1000003" % (3 * MIB, 7 * MIB + 1), "8 1 1 3"),
]


def test_writer_digest_runs_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "writer_sums_check")
    text = "".join(line + "\n" for line, _ in RUN_CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=120)
    _clean(r)
    got = r.stdout.splitlines()
    assert len(got) == len(RUN_CASES)
    for (line, want), g in zip(RUN_CASES, got):
        assert g == want, (line, g, want)
