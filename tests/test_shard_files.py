"""CPU: the storage entry points' file I/O (maxio_amd/csrc/shard_files.cpp:
whole-file reads and writes, the atomic replace of a healed shard, hex
digests, the pooled buffers, read_manifest) built on its own with
-fsanitize=address,undefined, as test_manifest_strict.py builds the manifest
reader, and run as a child process over a scratch directory
(tests/c_manifest/shard_files_check.cpp holds the checks)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from test_manifest_strict import ENV, HERE, ROOT, SAN


def test_shard_files_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "shard_files_check")
    csrc = os.path.join(ROOT, "maxio_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-o", exe,
                    os.path.join(HERE, "shard_files_check.cpp"), os.path.join(csrc, "shard_files.cpp"),
                    os.path.join(csrc, "manifest.cpp")], check=True)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    r = subprocess.run([exe, str(scratch)], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0 and "shard_files_check ok" in r.stdout, r.stdout + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
