"""The streaming CompleteMultipartUpload against the buffered driver, one lone
SSE upload at a time.

For each --mib (default 40 and 640): an upload of 8 MiB encrypted parts is
prepared once (frames under the upload key with part AADs, written by a child
process), then completed by mxec_complete_multipart_chunked_encrypted
(buffered) and by mxec_complete_multipart_streamed_encrypted (streamed) over
the same part files, 10 MiB chunks, m = 2.  Each mode runs in a fresh child
process: one small completion first, VmHWM noted, then --reps timed
completions (a host clock around the whole call; the directory is removed
between them), and VmHWM again: its growth is the host memory the mode took.
Peak host bytes are also counted from each path's own allocations, as
tools/reader_encrypted_bench.py counts them.

Every child runs under its own `timeout`, and the first one that fails ends
the run.

    python tools/multipart_stream_bench.py [--mib 40 640 --part-mib 8 --chunk-mib 10 --m 2 --reps 3]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UPLOAD_KEY, KEY, PREFIX = bytes(range(32, 64)), bytes(range(32)), b"\x80\x01\x02\x03"
UPLOAD_ID, AAD = "upl-bench", b"bucket\0key\0v\0"
FRAME, EXTRA, PIECE = 65536, 28, 1 << 20
LAUNCH = 16 * (FRAME + EXTRA)


def host_bytes(n: int, part: int, chunk: int, m: int) -> dict:
    """Each driver's largest host footprint for n plaintext bytes in encrypted parts of `part` bytes."""
    frames = (n + FRAME - 1) // FRAME
    stream = n + EXTRA * frames
    pframes = (min(part, n) + FRAME - 1) // FRAME
    # read_parts: the plaintext grows to n beside one part's file and AADs; then the plaintext, the whole
    # new frame stream with its AADs, and the m parity rows are all live
    buffered = max(n + min(part, n) + (EXTRA + 32) * pframes, n + stream + 32 * frames + m * chunk)
    # the writer: two pieces up, two down; the feed: two pieces of 16 frames, their AADs and statuses; a digest a chunk
    k = max(1, (stream + chunk - 1) // chunk)
    streamed = 4 * min(PIECE, max(chunk, 4096)) + 2 * LAUNCH + 2 * 16 * 36 + 4 * 16 * 32 + 64 * (k + m)
    return {"buffered_peak_host_bytes": buffered, "streamed_peak_host_bytes": streamed}


def hwm() -> int:
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmHWM:"):
                return int(line.split()[1]) * 1024
    return 0


def part_list(d: str) -> list[dict]:
    with open(os.path.join(d, "parts.json")) as f:
        return json.load(f)


def prepare(a) -> None:
    import numpy as np

    import maxio_amd

    n, part = a.mib[0] << 20, a.part_mib << 20
    block = np.random.default_rng(5).integers(0, 256, part, dtype=np.uint8)
    parts = []
    with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        for i, off in enumerate(range(0, n, part)):
            body = np.roll(block, i)[:min(part, n - off)]
            prefix = b"PART\0" + UPLOAD_ID.encode() + b"\0" + (i + 1).to_bytes(4, "little") + b"\0"
            aads = ctx.frame_aads(prefix, 0, (body.size + FRAME - 1) // FRAME)
            path = os.path.join(a.dir, "part%05d" % (i + 1))
            with open(path, "wb") as f:
                f.write(ctx.frames_encrypt(UPLOAD_KEY, b"UPLD", body, aads))
            parts.append({"path": path, "size": int(body.size), "etag": hashlib.md5(body.tobytes()).hexdigest(),
                          "part_number": i + 1, "encrypted": True})
    with open(os.path.join(a.dir, "parts.json"), "w") as f:
        json.dump(parts, f)


def mode(a) -> None:
    import maxio_amd

    chunk = a.chunk_mib << 20
    parts = part_list(a.dir)
    out = os.path.join(a.dir, a.mode + ".ec")
    with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        call = (ctx.complete_multipart_streamed_encrypted if a.mode == "streamed"
                else ctx.complete_multipart_chunked_encrypted)

        def complete(ps, c):
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.perf_counter()
            etag = call(out, c, a.m, ps, UPLOAD_KEY, UPLOAD_ID, KEY, PREFIX, AAD)
            return time.perf_counter() - t0, etag

        small = os.path.join(a.dir, "small_part")
        with open(parts[0]["path"], "rb") as f, open(small, "wb") as g:
            g.write(f.read(FRAME + EXTRA))
        complete([dict(parts[0], path=small, size=FRAME)], 1 << 16)  # the warm-up: kernels loaded, pools made
        before = hwm()
        walls, etag = [], None
        for _ in range(a.reps):
            w, etag = complete(parts, chunk)
            walls.append(w)
        growth = hwm() - before
        with open(os.path.join(out, "manifest.json"), "rb") as f:
            man = hashlib.sha256(f.read()).hexdigest()
        shutil.rmtree(out, ignore_errors=True)
    print(json.dumps({"mode": a.mode, "body_mib": a.mib[0], "part_mib": a.part_mib, "chunk_mib": a.chunk_mib, "m": a.m,
                      "wall_ms_median": round(1e3 * statistics.median(walls), 2),
                      "wall_ms": [round(1e3 * w, 2) for w in walls], "vmhwm_growth_bytes": growth, "etag": etag,
                      "manifest_sha256": man}))


def child(a, what: str, mib: int, d: str, limit: int) -> dict | None:
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--mode", what, "--mib", str(mib),
           "--part-mib", str(a.part_mib), "--chunk-mib", str(a.chunk_mib), "--m", str(a.m), "--reps", str(a.reps),
           "--dir", d]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write("%s (%d MiB) ended with %d\n%s" % (what, mib, r.returncode, r.stderr[-4000:]))
        return None
    lines = r.stdout.strip().splitlines()
    return json.loads(lines[-1]) if lines else {}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[40, 640])
    ap.add_argument("--part-mib", type=int, default=8)
    ap.add_argument("--chunk-mib", type=int, default=10)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--dir", default=None, help="where parts and objects are written (default: the temp dir)")
    ap.add_argument("--mode", choices=["prepare", "buffered", "streamed"], default=None)
    a = ap.parse_args()
    if a.mode == "prepare":
        prepare(a)
        return 0
    if a.mode:
        mode(a)
        return 0
    for mib in a.mib:
        d = tempfile.mkdtemp(prefix="multipart_stream_bench_", dir=a.dir)
        try:
            if child(a, "prepare", mib, d, a.limit) is None:
                return 1
            rows = {}
            for what in ("buffered", "streamed"):  # a fresh process each: its own VmHWM
                rows[what] = child(a, what, mib, d, a.limit)
                if rows[what] is None:
                    return 1
                print(json.dumps(rows[what]), flush=True)
            same = (rows["buffered"]["etag"] == rows["streamed"]["etag"] and
                    rows["buffered"]["manifest_sha256"] == rows["streamed"]["manifest_sha256"])
            row = {"body_mib": mib, "same_etag_and_manifest": same,
                   "streamed_over_buffered_wall": round(rows["streamed"]["wall_ms_median"] /
                                                        rows["buffered"]["wall_ms_median"], 3),
                   "streamed_over_buffered_vmhwm_growth": round(rows["streamed"]["vmhwm_growth_bytes"] /
                                                                max(1, rows["buffered"]["vmhwm_growth_bytes"]), 4)}
            row.update(host_bytes(mib << 20, a.part_mib << 20, a.chunk_mib << 20, a.m))
            print(json.dumps(row), flush=True)
            if not same:
                return 1
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
