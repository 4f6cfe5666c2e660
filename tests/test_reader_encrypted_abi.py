"""CPU: the streaming encrypted GET's entry points --
mxec_frames_decrypt_window_device and mxec_reader_open_encrypted -- are
declared the same way on every side of the boundary (header, linker map, Rust
crate, ctypes mirror, Python classes), and the reader's arithmetic
(maxio_amd/csrc/read_plan.hpp) keeps its promises when its rounds are played
over a model of the ring, run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Replaces: FrameDecryptor::for_range over VerifiedChunkReader (crypto.rs:186-420,
filesystem.rs:1618-1630, :1700-1725)."""
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
ARITY = {"mxec_frames_decrypt_window_device": 7, "mxec_reader_open_encrypted": 11}
NEW = list(ARITY)


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_new_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    p = _header_params("mxec_frames_decrypt_window_device")
    assert p[3] == "const mxec_frames_job* job" and p[4] == "uint64_t stream_off"
    assert p[5] == "const void* win" and p[6] == "int32_t* frame_status_dev"
    p = _header_params("mxec_reader_open_encrypted")
    assert p[1] == "const char* ec_dir" and p[2] == "const uint8_t key[32]"
    assert p[3].startswith("const uint8_t*") and p[4] == "uint32_t aad_prefix_len" and p[5] == "uint32_t frame_size"
    assert [x.split()[1] for x in p[6:10]] == ["plaintext_size", "offset", "length", "batch_bytes"]
    assert all(x.split()[0] == "uint64_t" for x in p[6:10]) and p[10] == "mxec_reader** out"
    # every entry point cites the reference it binds, and says what it promises
    text = open(HEADER).read()
    doc = text[text.index("mxec_reader_open_encrypted (get_object"):text.index("int mxec_reader_open_encrypted(")]
    assert "crypto.rs:186-420" in doc and "filesystem.rs:1618-1630" in doc
    for words in ("Failures stream", "never returned", "uploaded once", "frame index mismatch"):
        assert words in doc, words
    win = text[:text.index("int mxec_frames_decrypt_window_device(")][-1700:]
    assert "crypto.rs:186-420" in win and "Enqueue-only" in win and "exceed the window" in win


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
    m = re.search(r"pub fn mxec_reader_open_encrypted\((.*?)\)", block, flags=re.S)
    assert m.group(1).rstrip().endswith("out: *mut *mut MxecReader")  # the plain reader's handle type


def test_ctypes_mirror_and_python_classes():
    for name in NEW:
        res, args = _native._SIGS[name]
        assert len(args) == ARITY[name], name
        assert res is _native.INT, name
        assert hasattr(maxio_amd.lib(), name)
    assert callable(maxio_amd.Context.frames_decrypt_window_device)
    assert callable(maxio_amd.Context.open_reader_encrypted)
    import inspect

    sig = inspect.signature(maxio_amd.Context.open_reader_encrypted)
    assert list(sig.parameters)[1:] == ["ec_dir", "key", "aad_prefix", "offset", "length", "plaintext_size",
                                        "frame_size", "batch_bytes"]
    assert sig.parameters["frame_size"].default == 65536 and sig.parameters["batch_bytes"].default == 0
    sig = inspect.signature(maxio_amd.Context.frames_decrypt_window_device)
    assert list(sig.parameters)[1:] == ["job", "stream_off", "base_dev", "chunk_size", "slot_stride", "slots",
                                        "status_dev", "dev", "stream"]


# ---- the planner, stand-alone under the sanitizers ------------------------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_read_plan_under_sanitizers(tmp_path):
    """tests/c_manifest/read_plan_check.cpp plays the reader's rounds for chunk
    sizes 1, 7, 91, 92, 93, 101 and 2^20 against frame sizes 16, 64 and 65536,
    ranges at every frame edge, one chunk a round and more, lengths near 2^64,
    and checks at every step: each needed frame decrypted exactly once and not
    before its last byte is resident, no slot overwritten while a pending
    frame touches it, the ring bound."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "read_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", "read_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    m = re.fullmatch(r"ok (\d+) (\d+)\n", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) > 50000 and int(m.group(2)) > int(m.group(1))  # cases played, rounds in them
