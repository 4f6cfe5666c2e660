"""The streaming encrypted reader against the buffered encrypted GET, one lone
object read whole.

One SSE object (64 KiB frames, --chunk-mib chunks, m = --m) is written once,
then read whole in this process by mxec_get_object_chunked_encrypted into one
buffer (buffered) and through mxec_reader_open_encrypted in --read-mib reads
(reader), the two alternating: one untimed read of each, then --reps timed
reads of each.  The wall time of a read is a host clock around the whole call
or the whole open / read loop / close; both end with every byte on the host.
The SHA-256 of what each side returned is compared with the body's.

Peak host bytes are counted from each path's own allocations, not sampled: the
buffered call holds the whole ciphertext range (and the caller's whole
plaintext buffer); the reader holds three page-locked pieces of at most
1 MiB, one launch's AADs and statuses, and the caller's read buffer.

--batch-mib sets the reader's batch_bytes (0: its default, 64 MiB): a round
costs about one chunk's SHA-256 chain however many chunks it holds, so the
rounds a read takes set its wall time, and their size its HBM, not its host
bytes.

    python tools/reader_encrypted_bench.py [--mib 40 --chunk-mib 10 --m 2 --read-mib 1 --reps 5 --batch-mib 0]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEY, PREFIX, AAD = bytes(range(32)), b"\x80\x01\x02\x03", b"bucket\0key\0v\0"
FRAME, EXTRA = 65536, 28
PIECE = 1 << 20
DEFAULT_BATCH = 64 << 20


def host_bytes(n: int, chunk: int, read: int, batch: int) -> dict:
    """Each path's largest host footprint for a whole read of n plaintext bytes."""
    frames = (n + FRAME - 1) // FRAME
    stream = n + EXTRA * frames
    # mxec_get_object_chunked_encrypted: Bytes ct(ct_len + 1); a whole-frame range decrypts straight into `out`
    buffered = (stream + 1) + 32 * frames + n
    # the reader: two pieces up, one down, and per launch 32 B of AAD and 4 B of status a frame
    per_round = (batch or DEFAULT_BATCH) // chunk + 1
    slots = min((stream + chunk - 1) // chunk, per_round + (FRAME + EXTRA - 1) // chunk + 1)
    launch_frames = min(frames, slots * chunk // (FRAME + EXTRA) + 2)
    reader = 3 * min(PIECE, max(chunk, 4096)) + 36 * launch_frames + read
    return {"buffered_peak_host_bytes": buffered, "reader_peak_host_bytes": reader}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=40)
    ap.add_argument("--chunk-mib", type=int, default=10)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--read-mib", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-mib", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the object is written (default: the temp dir)")
    a = ap.parse_args()

    import numpy as np

    import maxio_amd

    n, chunk, read, batch = a.mib << 20, a.chunk_mib << 20, a.read_mib << 20, a.batch_mib << 20
    root = tempfile.mkdtemp(prefix="reader_enc_bench_", dir=a.dir)
    try:
        with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
            d = os.path.join(root, "o.ec")
            block = np.random.default_rng(3).integers(0, 256, 8 << 20, dtype=np.uint8)
            want = hashlib.sha256()
            w = ctx.open_writer_encrypted(d, chunk, a.m, n, KEY, PREFIX, AAD)
            for o in range(0, n, PIECE):
                piece = block[o % block.size:][:min(PIECE, n - o)]
                w.write(piece)
                want.update(piece.tobytes())
            w.finish()
            w.close()
            want = want.hexdigest()

            def buffered():
                t0 = time.perf_counter()
                out = ctx.get_object_chunked_encrypted(d, KEY, AAD, plaintext_size=n)
                wall = time.perf_counter() - t0
                return wall, hashlib.sha256(out).hexdigest()

            def reader():
                h = hashlib.sha256()
                pieces = []
                t0 = time.perf_counter()
                with ctx.open_reader_encrypted(d, KEY, AAD, plaintext_size=n, batch_bytes=batch) as r:
                    while True:
                        b = r.read(read)
                        if not b:
                            break
                        pieces.append(b)
                wall = time.perf_counter() - t0
                for b in pieces:  # hashed outside the timed span, as the buffered side's is
                    h.update(b)
                return wall, h.hexdigest()

            walls = {"buffered": [], "reader": []}
            for rep in range(a.reps + 1):  # the first of each is the warm-up
                for name, fn in (("buffered", buffered), ("reader", reader)):
                    wall, got = fn()
                    assert got == want, name + " returned other bytes than were written"
                    if rep:
                        walls[name].append(wall)
        row = {"body_mib": a.mib, "chunk_mib": a.chunk_mib, "m": a.m, "read_mib": a.read_mib, "batch_mib": a.batch_mib,
               "reps": a.reps}
        for name, ws in walls.items():
            row[name + "_wall_ms_median"] = round(1e3 * statistics.median(ws), 2)
            row[name + "_wall_ms"] = [round(1e3 * x, 2) for x in ws]
        row["reader_over_buffered_wall"] = round(row["reader_wall_ms_median"] / row["buffered_wall_ms_median"], 3)
        row.update(host_bytes(n, chunk, read, batch))
        print(json.dumps(row))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
