"""CPU: the streaming CompleteMultipartUpload's entry points --
mxec_frames_decrypt_ring_device, mxec_complete_multipart_streamed and
mxec_complete_multipart_streamed_encrypted -- are declared the same way on
every side of the boundary (header, linker map, Rust crate, ctypes mirror,
Python classes); they compile as C and resolve in the library; the argument
errors that are decided before a device is looked at come back without one;
and the feed's arithmetic (maxio_amd/csrc/part_plan.hpp) holds against a
byte-by-byte model, run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Replaces: complete_multipart_chunked (filesystem.rs:1147-1310) and
complete_multipart_chunked_encrypted (:1315-1560) over FrameDecryptor
(crypto.rs:186-420)."""
from __future__ import annotations

import ctypes
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
HERE = os.path.join(ROOT, "tests", "c_manifest")
ARITY = {"mxec_frames_decrypt_ring_device": 8, "mxec_complete_multipart_streamed": 8,
         "mxec_complete_multipart_streamed_encrypted": 14}
NEW = list(ARITY)
E_ARG, E_IO, E_INTEGRITY = -21, -40, -41


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_new_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    p = _header_params("mxec_frames_decrypt_ring_device")
    assert p[3] == "const mxec_frames_job* jobs" and p[4] == "uint64_t n_jobs"
    assert p[5] == "const uint64_t* ring_off" and p[6] == "const void* ring" and p[7] == "int32_t* frame_status_dev"
    p = _header_params("mxec_complete_multipart_streamed")
    assert p[4] == "const mxec_multipart_part* parts" and p[6] == "uint64_t window_bytes" and p[7] == "char etag_out[48]"
    buffered = _header_params("mxec_complete_multipart_chunked_encrypted")
    p = _header_params("mxec_complete_multipart_streamed_encrypted")
    assert p[:12] == buffered[:12] and p[12] == "uint64_t window_bytes" and p[13] == buffered[12]
    text = open(HEADER).read()
    m = re.search(r"struct mxec_frames_ring \{(.*?)\};\s*typedef struct mxec_frames_ring mxec_frames_ring;", text, flags=re.S)
    assert m, "mxec_frames_ring not declared"
    fields = re.findall(r"(\w[\w\* ]*?)\s*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert [(" ".join(t.split()), n) for t, n in fields] == [("uint8_t*", "base_dev"), ("uint64_t", "bytes")]
    # every entry point cites the reference it binds
    ring = text[:text.index("struct mxec_frames_ring {")][-2200:]
    assert "crypto.rs:186-420" in ring and "filesystem.rs:1375-1387" in ring
    doc = text[text.index("The two completions above as streams"):text.index("int mxec_complete_multipart_streamed(")]
    assert "filesystem.rs:1375-1387" in doc and "mxec_frames_len(size, 65536)" in doc


def test_map_exports_them():
    text = open(os.path.join(ROOT, "maxio_amd", "csrc", "maxio_ec.map")).read()
    glob = re.search(r"global:\s*([^;]+);", text).group(1).split()
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, g) for g in glob), name
    out = subprocess.run(["nm", "-D", "--defined-only", maxio_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s$" % name, out, re.M), name
    # the writer's feed is internal: nothing of it is exported
    assert "writer_feed" not in out and "multipart_etag" not in out


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "rust", "maxio-ec-sys", "src", "lib.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S).group(1)
    for name in NEW:
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, block, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == ARITY[name], name
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\(Clone, Copy\)\]\s*pub struct MxecFramesRing \{(.*?)\}", src, flags=re.S)
    assert m, "MxecFramesRing"
    assert re.findall(r"pub (\w+): ([^,]+),", m.group(1)) == [("base_dev", "*mut u8"), ("bytes", "u64")]


def test_ctypes_mirror_and_python_classes():
    import inspect

    for name in NEW:
        res, args = _native._SIGS[name]
        assert len(args) == ARITY[name], name
        assert res is _native.INT, name
        assert hasattr(maxio_amd.lib(), name)
    r = _native.FramesRing
    assert [n for n, _ in r._fields_] == ["base_dev", "bytes"]
    assert ctypes.sizeof(r) == 16 and r.bytes.offset == 8
    sig = inspect.signature(maxio_amd.Context.frames_decrypt_ring_device)
    assert list(sig.parameters)[1:] == ["jobs", "ring_offs", "base_dev", "ring_bytes", "status_dev", "dev", "stream"]
    for name, buffered in (("complete_multipart_streamed", "complete_multipart_chunked"),
                           ("complete_multipart_streamed_encrypted", "complete_multipart_chunked_encrypted")):
        got = list(inspect.signature(getattr(maxio_amd.Context, name)).parameters)
        assert got == list(inspect.signature(getattr(maxio_amd.Context, buffered)).parameters) + ["window_bytes"]
        assert inspect.signature(getattr(maxio_amd.Context, name)).parameters["window_bytes"].default == 0


def test_compiles_as_c_and_resolves(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "multipart_streamed_abi_check")
    libdir = os.path.dirname(maxio_amd.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "multipart_streamed_abi_check.c"), "-L" + libdir, "-lmaxio_ec",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "multipart_streamed abi ok" in r.stdout


def _err():
    return maxio_amd.lib().mxec_last_error().decode()


def _parts(specs):
    arr = (_native.MultipartPart * max(1, len(specs)))()
    for i, (path, size, enc) in enumerate(specs):
        arr[i].path = path.encode()
        arr[i].size = size
        arr[i].part_number = i + 1
        arr[i].encrypted = enc
    return arr


def test_argument_errors_that_need_no_device(tmp_path):
    """Everything that is decided before the writer opens comes back without a
    context: nothing is created."""
    lib = maxio_amd.lib()
    etag = ctypes.create_string_buffer(48)
    key = (ctypes.c_uint8 * 32)()
    pre = (ctypes.c_uint8 * 4)()
    ec = str(tmp_path / "x.ec")
    plain = tmp_path / "plain"
    plain.write_bytes(b"p" * 1000)
    short = tmp_path / "short"
    short.write_bytes(b"s" * (65536 + 28 + 5 + 27))  # FS + 5 bytes of plaintext need FS + 28 + 5 + 28
    nope = str(tmp_path / "nope")

    def run_plain(specs, n=None):
        return lib.mxec_complete_multipart_streamed(None, ec.encode(), 4096, 2, _parts(specs), len(specs) if n is None else n,
                                                    0, etag)

    def run_enc(specs, upload_key=key, upload_id=b"upl"):
        return lib.mxec_complete_multipart_streamed_encrypted(None, ec.encode(), 4096, 2, _parts(specs), len(specs),
                                                              upload_key, upload_id, key, pre, None, 0, 0, etag)

    assert lib.mxec_complete_multipart_streamed(None, ec.encode(), 4096, 2, None, 1, 0, etag) == E_ARG
    assert lib.mxec_complete_multipart_streamed(None, ec.encode(), 4096, 2, _parts([]), 0, 0, None) == E_ARG
    assert run_plain([(str(plain), 1000, 1)]) == E_ARG and "encrypted part: use the _encrypted driver" in _err()
    assert run_plain([(str(plain), 1000, 0), (nope, 5, 0)]) == E_IO and "nope" in _err()
    assert run_enc([(str(plain), 1000, 0), (nope, 5, 1)]) == E_IO
    assert run_enc([(str(plain), 900, 1)], upload_key=None) == E_ARG and "encrypted part without upload key" in _err()
    assert run_enc([(str(plain), 900, 1)], upload_id=None) == E_ARG and "encrypted part without upload key" in _err()
    assert run_enc([(str(plain), 1000, 0), (str(short), 65536 + 5, 1)]) == E_INTEGRITY
    assert "truncated encrypted frame" in _err()
    assert lib.mxec_complete_multipart_streamed_encrypted(None, ec.encode(), 4096, 2, _parts([]), 0, key, b"upl", None,
                                                          pre, None, 0, 0, etag) == E_ARG
    # with nothing left to refuse the writer is opened, and that needs the context
    assert run_plain([(str(plain), 1000, 0)]) == E_ARG and "null argument" in _err()
    assert run_enc([(str(plain), 972, 1)]) == E_ARG and "null argument" in _err()
    assert not os.path.exists(ec)

    # the ring form: every check comes before the device is opened
    ring = _native.FramesRing(0x1000, 300)
    job = (_native.FramesJob * 2)()
    k32 = (ctypes.c_uint8 * 32)()
    for j in job:
        j.key = ctypes.addressof(k32)
        j.frame_size = 64
        j.in_dev = 0x2000
        j.len = 128
    offs = (ctypes.c_uint64 * 2)(0, 128)
    st = ctypes.c_void_p(0x3000)

    def run_ring(n=2, jobs=job, o=offs, r=ring, s=st):
        return lib.mxec_frames_decrypt_ring_device(None, 0, None, jobs, n, o, ctypes.byref(r) if r is not None else None, s)

    assert run_ring(n=0, jobs=None, o=None, r=None, s=None) == 0
    assert run_ring(jobs=None) == E_ARG and run_ring(o=None) == E_ARG and run_ring(r=None) == E_ARG
    assert run_ring(s=None) == E_ARG and "null argument" in _err()
    assert run_ring(r=_native.FramesRing(0, 300)) == E_ARG
    assert run_ring(r=_native.FramesRing(0x1000, 0)) == E_ARG and "ring bytes" in _err()
    assert run_ring(o=(ctypes.c_uint64 * 2)(0, 300)) == E_ARG and "ring_off" in _err()
    assert run_ring(r=_native.FramesRing(0x1000, 255)) == E_ARG and "overwrite itself" in _err()
    job[1].frame_size = 24
    assert run_ring() == E_ARG and "frame_size" in _err()
    job[1].frame_size = 2 ** 31
    assert run_ring() == E_ARG and "frame_size" in _err()
    job[1].frame_size = 64
    job[1].aad_len = 32
    assert run_ring() == E_ARG and "null argument" in _err()
    job[1].aad_len = 0
    job[0].key = None
    assert run_ring() == E_ARG and "null argument" in _err()
    job[0].key = ctypes.addressof(k32)
    # what is left needs the context
    assert run_ring() == E_ARG and "null context" in _err()


SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_part_plan_under_sanitizers(tmp_path):
    """tests/c_manifest/part_plan_check.cpp: the empty list, parts of 0 and 1
    bytes, 65535 / 65536 / 65537, multiples of 64 KiB and not, 40 one-byte
    parts, plain and encrypted alternating, bodies that wrap the ring several
    times; every plaintext byte once at (body offset) % ring, no launch over
    16 frames or over the ring, launches <= ceil(frames / 16) + transitions + 1."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "part_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(HERE, "part_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"^part_plan ok: \d+ cases$", r.stdout, re.M), r.stdout
