"""CPU: the streaming PUT's entry points -- mxec_encode_update_strided_device
and mxec_writer_open / _write / _finish / _close -- are declared the same way
on every side of the boundary (header, linker map, Rust crate, ctypes mirror,
Python classes), and the writer's arithmetic (maxio_amd/csrc/writer_plan.hpp)
does what the header documents, run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Replaces: put_object_chunked's read loop (filesystem.rs:686-773); the update
call replaces nothing in the crate (filesystem.rs:1121-1124 computes parity
once every chunk is on disk)."""
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
ARITY = {"mxec_encode_update_strided_device": 19, "mxec_writer_open": 8, "mxec_writer_write": 3,
         "mxec_writer_finish": 1, "mxec_writer_close": 1}
NEW = list(ARITY)


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_new_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    p = _header_params("mxec_encode_update_strided_device")
    assert p[7] == "int first" and p[8] == "int count"
    assert p[9].startswith("const uint8_t*") and p[12].startswith("const uint64_t*")
    assert p[13].startswith("const uint8_t*") and p[16].startswith("uint8_t*")
    p = _header_params("mxec_writer_open")
    assert [x.split()[0] for x in p[2:7]] == ["uint64_t", "uint32_t", "uint64_t", "uint64_t", "uint64_t"]
    assert _header_params("mxec_writer_write")[1].startswith("const uint8_t*")
    text = open(HEADER).read()
    assert "typedef struct mxec_writer mxec_writer;" in text
    # every entry point cites the reference it binds
    doc = text[text.index("put_object_chunked (filesystem.rs:686-773) as a push stream"):text.index("typedef struct mxec_writer")]
    for name in ("mxec_writer_open", "mxec_writer_write", "mxec_writer_finish", "mxec_writer_close"):
        assert name in doc
    assert doc.count("filesystem.rs:") >= 4
    upd = text[:text.index("int mxec_encode_update_strided_device")][-1500:]
    assert "filesystem.rs:1121-1124" in upd and "replaces nothing" in upd


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
        m = re.search(r"pub fn %s\((.*?)\)\s*(->\s*c_int)?;" % name, block, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == ARITY[name], name
        assert bool(m.group(2)) == (name != "mxec_writer_close"), name


def test_ctypes_mirror_and_python_classes():
    for name in NEW:
        res, args = _native._SIGS[name]
        assert len(args) == ARITY[name], name
        assert res is (None if name == "mxec_writer_close" else _native.INT), name
    assert hasattr(maxio_amd.lib(), "mxec_writer_open")
    assert callable(maxio_amd.Context.encode_update_strided_device)
    assert callable(maxio_amd.Context.open_writer)
    for meth in ("write", "finish", "close", "__enter__", "__exit__"):
        assert callable(getattr(maxio_amd.ChunkWriter, meth)), meth
    assert "ChunkWriter" in maxio_amd.__all__


# ---- the planner, stand-alone under the sanitizers ------------------------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
U64 = 2 ** 64 - 1

# (case line, answer line).  Runs are chunk:at:src:len:opens:completes.
CASES = [
    # k, the last chunk's length, window slots
    ("plan 100 0 0", "1 0 1"),                      # an empty body: one empty chunk
    ("plan 100 1 0", "1 1 1"),
    ("plan 100 100 0", "1 100 1"),
    ("plan 100 101 0", "2 1 2"),
    ("plan 100 1000 0", "10 100 4"),                # default window: four chunks
    ("plan 100 1000 100", "10 100 2"),              # at least two chunks are used
    ("plan 100 1000 399", "10 100 3"),
    ("plan 100 1000 100000", "10 100 10"),          # never more than k
    ("plan 1 %d 0" % U64, "%d 1 4" % U64),          # no overflow in ceil
    ("plan 2 %d 0" % U64, "%d 1 4" % 2 ** 63),
    ("plan %d %d 0" % (U64, U64), "1 %d 1" % U64),
    ("plan %d %d 0" % (U64 - 1, U64), "2 1 2"),
    ("plan 3 %d 0" % (U64 - 1), "%d 2 4" % ((U64 - 2) // 3 + 1)),
    # a write within one chunk
    ("cut 100 250 0 0 40", "0:0:0:40:1:0"),
    ("cut 100 250 0 40 40", "0:40:0:40:0:0"),
    ("cut 100 250 0 40 60", "0:40:0:60:0:1"),       # an exact fill of the chunk
    # crossing one boundary, several, and ending the body
    ("cut 100 250 0 40 100", "0:40:0:60:0:1 1:0:60:40:1:0"),
    ("cut 100 250 0 0 250", "0:0:0:100:1:1 1:0:100:100:1:1 2:0:200:50:1:1"),
    ("cut 100 250 0 99 151", "0:99:0:1:0:1 1:0:1:100:1:1 2:0:101:50:1:1"),
    ("cut 100 250 0 200 50", "2:0:0:50:1:1"),       # the short last chunk completes at 50
    ("cut 100 250 0 249 1", "2:49:0:1:0:1"),
    ("cut 100 300 0 200 100", "2:0:0:100:1:1"),     # total_len a multiple of the chunk size
    # zero-length writes: at the start, mid-chunk, on a boundary, at the end, of an empty body
    ("cut 100 250 0 0 0", "-"),
    ("cut 100 250 0 40 0", "-"),
    ("cut 100 250 0 100 0", "-"),
    ("cut 100 250 0 250 0", "-"),
    ("cut 100 0 0 0 0", "-"),
    # over-run by one, from several positions; nothing is taken
    ("cut 100 250 0 0 251", "overrun: write of 251 bytes at 0 runs past the 250 declared bytes"),
    ("cut 100 250 0 249 2", "overrun: write of 2 bytes at 249 runs past the 250 declared bytes"),
    ("cut 100 250 0 250 1", "overrun: write of 1 bytes at 250 runs past the 250 declared bytes"),
    ("cut 100 0 0 0 1", "overrun: write of 1 bytes at 0 runs past the 0 declared bytes"),
    ("cut 100 250 0 1 %d" % U64, "overrun: write of %d bytes at 1 runs past the 250 declared bytes" % U64),
    # just below 2^64
    ("cut %d %d 0 %d 2" % (2 ** 63, U64, 2 ** 63 - 1), "0:%d:0:1:0:1 1:0:1:1:1:0" % (2 ** 63 - 1)),
    # 2^64 - 1 = 7 q + 1: chunk q - 1 ends at 7 q, the last chunk holds one byte
    ("cut 7 %d 0 %d 3" % (U64, U64 - 3), "%d:5:0:2:0:1 %d:0:2:1:1:1" % ((U64 - 1) // 7 - 1, (U64 - 1) // 7)),
    ("cut 7 %d 0 %d 4" % (U64, U64 - 3),
     "overrun: write of 4 bytes at %d runs past the %d declared bytes" % (U64 - 3, U64)),
    # finish: exact, short by one, short by all, an empty body
    ("end 100 250 250", "ok"),
    ("end 100 250 249", "body ended at 249 of 250 declared bytes"),
    ("end 100 250 0", "body ended at 0 of 250 declared bytes"),
    ("end 100 0 0", "ok"),
    ("end 1 %d %d" % (U64, U64 - 1), "body ended at %d of %d declared bytes" % (U64 - 1, U64)),
    # slot reuse order: chunk j takes slot j % slots once chunk j - slots is done with
    ("slots 100 700 200 7", "0/- 1/- 0/0 1/1 0/2 1/3 0/4"),
    ("slots 100 700 300 7", "0/- 1/- 2/- 0/0 1/1 2/2 0/3"),
    ("slots 100 150 300 2", "0/- 1/-"),             # a window larger than the body: no chunk ever waits
]


def test_writer_plan_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "writer_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", "writer_plan_check.cpp")], check=True)
    text = "".join(line + "\n" for line, _ in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    for (line, want), g in zip(CASES, got):
        assert g == want, (line, g, want)
