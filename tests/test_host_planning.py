"""CPU unit tests of host-side planning helpers, built with
-fsanitize=address,undefined:

* the SHA-256 stream form is refused when its 32-bit item counter could
  wrap (many short messages plus one very long one would leave
  the tail items unhashed and their ok flags stale);
* mxec_encode_batch_host deals a mixed batch over devices by bytes (within
  10 % per device at 2/4/8 devices) and a uniform one as object o -> o mod D
  (VERDICT r2 item 6);
* the piece grid of the piece-major host waves tiles every message with
  and without a ramp and after widening mid-wave (piece_grid.hpp);
* the wave cutter of the host batch calls keeps every object in exactly one
  wave, in order, within the pool allowance unless alone (wave_cut.hpp);
* the Reed-Solomon launch planner lays out the descriptor tables of the
  uniform, unaligned, grouped, verify / locate and multi-r launches so that a
  walk of each launch meets every (object, tile) once on that object's
  entries, and splits a mixed call into grouped, uniform and multi-r launches
  by its alignment, uniformity and 32-bit rules (rs_plan.hpp);
* the reconstructs' decode table builder puts every object with shards to
  rebuild exactly once under its number of rebuilt shards, its rows inside the
  returned tables with the windowed pointers, lengths and shard size, for both
  shard-location forms (decode_tables.hpp);
* the host GF(2^8) algebra (gf256.cpp: the v_perm coefficient tables, the
  encoding matrix, the decode plans) equals the oracle's at the wide shapes
  of test_wide_stripes_gpu.py and at 256 shards (gf256_check.cpp, built with
  gf256.cpp; the oracle's C sources are compiled beside it as plain -O2
  objects: they are the checker, and instrumented they take a minute)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "c_manifest")
# What a check is built from besides its own file: product sources under the
# sanitizers with it, oracle sources as plain objects.
WITH = {"gf256_check.cpp": {"cpp": ["maxio_amd/csrc/gf256.cpp"],
                            "oracle": ["oracle/rs_oracle.c", "oracle/sha256_oracle.c"]}}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("src,ok", [("sha_guard_check.cpp", "sha guard ok"), ("deal_check.cpp", "deal ok"),
                                    ("piece_grid_check.cpp", "piece grid ok"), ("wave_cut_check.cpp", "wave cut ok"),
                                    ("rs_plan_check.cpp", "rs plan ok"),
                                    ("decode_tables_check.cpp", "decode tables ok"),
                                    ("gf256_check.cpp", "gf256 ok")])
def test_host_planning(tmp_path, src, ok):
    exe = str(tmp_path / src.split(".")[0])
    more = [os.path.join(ROOT, p) for p in WITH.get(src, {}).get("cpp", [])]
    for p in WITH.get(src, {}).get("oracle", []):
        more.append(str(tmp_path / (os.path.basename(p) + ".o")))
        subprocess.run(["g++", "-x", "c", "-std=c11", "-O2", "-c", os.path.join(ROOT, p), "-o", more[-1]], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, src)] + more + ["-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert ok in r.stdout
