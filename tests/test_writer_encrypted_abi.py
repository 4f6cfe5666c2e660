"""CPU: the streaming encrypted PUT's entry points --
mxec_frames_encrypt_window_device and mxec_writer_open_encrypted -- are
declared the same way on every side of the boundary (header, linker map, Rust
crate, ctypes mirror, Python classes), and the writer's arithmetic
(maxio_amd/csrc/frame_plan.hpp, with the host SHA-256 of its frame AADs) does
what the header documents, run as a stand-alone program under
-fsanitize=address,undefined.  No kernel is launched here.

Replaces: put_object_chunked_encrypted's read loop (filesystem.rs:835-1060)
over FrameEncryptor (crypto.rs:94-117)."""
from __future__ import annotations

import ctypes
import fnmatch
import hashlib
import os
import re
import shutil
import subprocess

import pytest

import maxio_amd
from maxio_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxio_ec.h")
ARITY = {"mxec_frames_encrypt_window_device": 6, "mxec_writer_open_encrypted": 12}
NEW = list(ARITY)


def _header_params(name: str) -> list[str]:
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} not declared in the header"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_new_symbols():
    for name in NEW:
        assert len(_header_params(name)) == ARITY[name], name
    p = _header_params("mxec_frames_encrypt_window_device")
    assert p[3] == "const mxec_frames_job* job" and p[4] == "uint64_t stream_off"
    assert p[5] == "const void* win"  # a mxec_frames_window, as mxec_scrub_object passes its report
    p = _header_params("mxec_writer_open_encrypted")
    assert [x.split()[0] for x in p[2:5]] == ["uint64_t", "uint32_t", "uint64_t"]
    assert p[5] == "const uint8_t key[32]" and p[6] == "const uint8_t nonce_prefix[4]"
    assert p[7].startswith("const uint8_t*") and p[8] == "uint32_t aad_prefix_len"
    assert p[9] == "uint64_t window_bytes" and p[10] == "uint32_t which" and p[11] == "void** out"
    text = open(HEADER).read()
    m = re.search(r"struct mxec_frames_window \{(.*?)\};\s*typedef struct mxec_frames_window mxec_frames_window;", text,
                  flags=re.S)
    assert m, "mxec_frames_window not declared"
    fields = re.findall(r"(\w[\w\* ]*?)\s*(\w+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert [(" ".join(t.split()), n) for t, n in fields] == [
        ("uint8_t*", "base_dev"), ("uint64_t", "chunk_size"), ("uint64_t", "slot_stride"), ("uint64_t", "slots")]
    # every entry point cites the reference it binds
    doc = text[text.index("mxec_writer_open_encrypted (put_object_chunked_encrypted"):
               text.index("typedef struct mxec_writer mxec_writer")]
    assert "filesystem.rs:835-1060" in doc and "crypto.rs" in doc
    win = text[:text.index("struct mxec_frames_window {")][-1900:]
    assert "filesystem.rs:835-1060" in win and "crypto.rs" in win


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
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\(Clone, Copy\)\]\s*pub struct MxecFramesWindow \{(.*?)\}", src, flags=re.S)
    assert m, "MxecFramesWindow"
    assert re.findall(r"pub (\w+): ([^,]+),", m.group(1)) == [
        ("base_dev", "*mut u8"), ("chunk_size", "u64"), ("slot_stride", "u64"), ("slots", "u64")]


def test_ctypes_mirror_and_python_classes():
    for name in NEW:
        res, args = _native._SIGS[name]
        assert len(args) == ARITY[name], name
        assert res is _native.INT, name
    assert hasattr(maxio_amd.lib(), "mxec_writer_open_encrypted")
    assert hasattr(maxio_amd.lib(), "mxec_frames_encrypt_window_device")
    w = _native.FramesWindow
    assert [n for n, _ in w._fields_] == ["base_dev", "chunk_size", "slot_stride", "slots"]
    assert ctypes.sizeof(w) == 32 and w.slots.offset == 24
    assert callable(maxio_amd.Context.frames_encrypt_window_device)
    assert callable(maxio_amd.Context.open_writer_encrypted)


# ---- the planner, stand-alone under the sanitizers ------------------------------------------------

SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
U64 = 2 ** 64 - 1
FP, FL = 65536, 65564  # a frame's plaintext and its bytes in the stream
MIB = 1 << 20
N4 = 3 * FP + 777      # three whole frames and a short one


def _frames(n):
    return (n + FP - 1) // FP


def _largest_plain():
    """The largest plaintext whose frame stream still fits in 64 bits."""
    lo, hi = 0, U64  # p + 28 * frames(p) grows with p: bisect
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid + 28 * _frames(mid) <= U64:
            lo = mid
        else:
            hi = mid - 1
    return lo


BIG = _largest_plain()


def _ring(c, slots, off, n):
    """The mapping, chunk by chunk: slot:at:src:len."""
    out, src = [], 0
    while src < n:
        x = off + src
        step = min(n - src, c - x % c)
        out.append("%d:%d:%d:%d" % ((x // c) % slots, x % c, src, step))
        src += step
    return " ".join(out) or "-"


def _run(r, plain):
    pl = min(MIB, plain - r * MIB)
    nf = _frames(pl)
    return "%d:%d:%d:%d:%d:%d:%d" % (r, 16 * r, nf, pl, 16 * r * FL, pl + 28 * nf, int((r + 1) * MIB >= plain))


# (case line, answer line)
CASES = [
    # frames and stream bytes of a plaintext
    ("len 0", "0 0"),                                  # an empty body: no frame at all
    ("len 1", "1 29"),
    ("len %d" % (FP - 1), "1 %d" % (FP + 27)),
    ("len %d" % FP, "1 %d" % FL),
    ("len %d" % (FP + 1), "2 %d" % (FL + 29)),
    ("len %d" % N4, "4 %d" % (N4 + 112)),
    ("len %d" % BIG, "%d %d" % (_frames(BIG), BIG + 28 * _frames(BIG))),   # no overflow just below ...
    ("len %d" % (BIG + 1), "overflow"),                                     # ... and said so above
    ("len %d" % U64, "overflow"),
    # frame f's place in the stream, its bytes there and its plaintext
    ("frame %d 0" % N4, "0 %d %d" % (FL, FP)),
    ("frame %d 2" % N4, "%d %d %d" % (2 * FL, FL, FP)),
    ("frame %d 3" % N4, "%d %d %d" % (3 * FL, 777 + 28, 777)),             # the short last frame
    ("frame %d 0" % 1, "0 29 1"),
    ("frame %d %d" % (BIG, _frames(BIG) - 1),
     "%d %d %d" % ((_frames(BIG) - 1) * FL, BIG - (_frames(BIG) - 1) * FP + 28, BIG - (_frames(BIG) - 1) * FP)),
    # frames that become whole: a write that ends one byte before, on and after a frame boundary
    ("due %d 0 %d" % (N4, FP - 1), "0 0"),
    ("due %d 0 %d" % (N4, FP), "0 1"),
    ("due %d 0 %d" % (N4, FP + 1), "0 1"),
    ("due %d %d %d" % (N4, FP - 1, FP), "0 1"),
    ("due %d %d %d" % (N4, FP, FP + 1), "1 0"),
    ("due %d %d %d" % (N4, FP + 1, 3 * FP), "1 2"),
    ("due %d %d %d" % (N4, 3 * FP, N4 - 1), "3 0"),    # the short last frame goes with the body's last byte
    ("due %d %d %d" % (N4, N4 - 1, N4), "3 1"),
    ("due %d 0 %d" % (N4, N4), "0 4"),
    ("due %d %d %d" % (2 * FP, FP, 2 * FP), "1 1"),    # a body that ends on a frame boundary
    ("due 0 0 0", "0 0"),                              # an empty body
    ("due %d %d %d" % (BIG, BIG - 1, BIG), "%d 1" % (_frames(BIG) - 1)),
    # the launches: one per MiB of plaintext, due with its last byte or the body's
    ("runs %d 0 %d" % (2 * MIB + 5, MIB - 1), "-"),
    ("runs %d 0 %d" % (2 * MIB + 5, MIB), _run(0, 2 * MIB + 5)),
    ("runs %d %d %d" % (2 * MIB + 5, MIB - 1, MIB + 1), _run(0, 2 * MIB + 5)),
    ("runs %d %d %d" % (2 * MIB + 5, MIB, 2 * MIB + 4), _run(1, 2 * MIB + 5)),
    ("runs %d %d %d" % (2 * MIB + 5, 2 * MIB, 2 * MIB + 5), _run(2, 2 * MIB + 5)),
    ("runs %d 0 %d" % (2 * MIB + 5, 2 * MIB + 5), " ".join(_run(r, 2 * MIB + 5) for r in range(3))),
    ("runs %d %d %d" % (N4, 4099 * 3, 4099 * 4), "-"),  # a small write completes a frame at the most: no launch
    ("runs %d %d %d" % (N4, N4 - 1, N4), _run(0, N4)),
    ("runs %d 0 %d" % (2 * MIB, 2 * MIB), _run(0, 2 * MIB) + " " + _run(1, 2 * MIB)),
    ("runs 0 0 0", "-"),
    ("runs %d %d %d" % (BIG, BIG - 1, BIG), _run((BIG - 1) // MIB, BIG)),
    # ring stretches: inside one chunk, across one boundary, across several, across the wrap, ending on a boundary
    ("ring 100000 4 100 50", "0:100:0:50"),
    ("ring 100 4 90 20", "0:90:0:10 1:0:10:10"),
    ("ring 100 4 390 20", "3:90:0:10 0:0:10:10"),      # the wrap
    ("ring 100 4 150 50", "1:50:0:50"),                # ends exactly on a boundary: no empty stretch after it
    ("ring 100 4 100 100", "1:0:0:100"),
    ("ring 100 4 7 0", "-"),
    ("ring 7 3 %d %d" % (FL, FL), _ring(7, 3, FL, FL)),                    # 9 367 cuts in one frame
    ("ring 20000 2 %d %d" % (FL, FL), _ring(20000, 2, FL, FL)),
    ("ring 20000 5 %d %d" % (3 * FL, 777 + 28), _ring(20000, 5, 3 * FL, 777 + 28)),
    ("ring %d 2 %d 10" % (2 ** 63, U64 - 9), "1:%d:0:10" % (2 ** 63 - 10)),  # the stream's last bytes below 2^64
    ("ring 1 1 %d 3" % (U64 - 3), "0:0:0:1 0:0:1:1 0:0:2:1"),
    # the chunks a stream range completes
    ("done 100 250 0 100", "0 1"),
    ("done 100 250 0 99", "0 0"),
    ("done 100 250 40 100", "0 1"),
    ("done 100 250 150 100", "1 2"),                   # the short last chunk completes with the stream
    ("done 100 250 200 49", "2 0"),
    ("done 100 300 200 100", "2 1"),
    ("done 20000 %d %d %d" % (N4 + 112, FL, 2 * FL), "%d %d" % (FL // 20000, 3 * FL // 20000 - FL // 20000)),
    ("done 100 0 0 0", "0 0"),                         # the empty body's one chunk is finish()'s
]
for _prefix in (b"", b"bucket\0key\0v1\0", bytes(range(47)), bytes(range(48)), bytes(range(56)), bytes(range(120))):
    for _idx in (0, 2 ** 32, U64):
        CASES.append(("aad %s %d" % (_prefix.hex() or "-", _idx),
                      hashlib.sha256(_prefix + _idx.to_bytes(8, "little")).hexdigest()))


def test_frame_plan_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "frame_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", exe,
                    os.path.join(ROOT, "tests", "c_manifest", "frame_plan_check.cpp")], check=True)
    text = "".join(line + "\n" for line, _ in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    for (line, want), g in zip(CASES, got):
        assert g == want, (line[:80], g[:200], want[:200])
