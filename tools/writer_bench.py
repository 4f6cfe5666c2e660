"""Streaming writer against the buffered PUT for one lone object.

One body in page-locked memory (mxec_host_alloc), written either by
mxec_put_object_chunked in one call or through mxec_writer_* in --call-mib
pieces.  Each side runs in a fresh process so that its host memory is its
own: the process opens a context, allocates and fills the body, runs a PUT
of four 64 KiB chunks the same way (the runtime loads its code objects and
sets its queues up there, hundreds of MB that are not the call's), notes its
resident set, runs the PUT once while a thread samples the resident set
every 0.2 ms -- the highest sample less the note is the peak of host bytes
the library allocated for the call, page-locked and pageable alike; the
caller's body is resident before the note -- then times --reps more PUTs.
Prints one JSON line per side and one with the ratios.

--sums WHICH (MXEC_SUM_* bits, e.g. 1 = MD5): both sides also produce the body
digests, the writer through mxec_writer_open_sums / mxec_writer_sums, the
buffered side through mxec_put_object_chunked_sums (MD5 and at most one
checksum).  The digests are checked against hashlib once, outside the timing.

    python tools/writer_bench.py [--mib 40 --chunk-mib 10 --m 2 --call-mib 1 --reps 7 --sums 0]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resident() -> int:
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


class PeakResident:
    """The highest resident set seen while the block runs."""

    def __enter__(self):
        self.peak, self._stop = resident(), threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop.wait(0.0002):
            self.peak = max(self.peak, resident())

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, resident())


def side(a) -> None:
    import numpy as np

    import maxio_amd

    n, c, piece = a.mib << 20, a.chunk_mib << 20, a.call_mib << 20
    root = tempfile.mkdtemp(prefix="writer_bench_", dir=a.dir)
    try:
        with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
            body = ctx.host_array(n)
            body[:] = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)

            algo = {0: None, 2: "CRC32", 4: "CRC32C", 8: "SHA1", 16: "SHA256"}.get(a.sums & ~1)
            last = {}

            def put(d, n=n, c=c):
                t0 = time.perf_counter()
                if a.side == "buffered":
                    if a.sums:
                        last["etag"] = ctx.put_object_chunked_sums(d, c, a.m, body[:n], algo)["etag"]
                    else:
                        ctx.put_object_chunked(d, c, a.m, body[:n])
                    return time.perf_counter() - t0, 0.0
                w = ctx.open_writer(d, c, a.m, n, which=a.sums)
                for o in range(0, n, piece):
                    w.write(body[o:min(n, o + piece)])
                t1 = time.perf_counter()
                w.finish()
                sums = w.sums()
                w.close()
                if "md5" in sums:
                    last["etag"] = '"%s"' % sums["md5"].hex()
                return time.perf_counter() - t0, time.perf_counter() - t1

            put(os.path.join(root, "warm.ec"), n=4 << 16, c=1 << 16)
            before = resident()
            with PeakResident() as pr:
                put(os.path.join(root, "first.ec"))
            peak = pr.peak - before
            walls, tails = [], []
            for r in range(a.reps):
                wall, tail = put(os.path.join(root, "r%d.ec" % r))
                walls.append(wall)
                tails.append(tail)
            if a.sums & 1:
                import hashlib

                assert last["etag"] == '"%s"' % hashlib.md5(body.tobytes()).hexdigest(), "ETag mismatch"
            ctx.host_free(body)
        print(json.dumps({"side": a.side, "sums": a.sums, "body_mib": a.mib, "chunk_mib": a.chunk_mib, "m": a.m,
                          "call_mib": a.call_mib, "wall_ms_median": round(1e3 * statistics.median(walls), 2),
                          "wall_ms_min": round(1e3 * min(walls), 2), "wall_ms": [round(1e3 * w, 2) for w in walls],
                          "finish_close_ms_median": round(1e3 * statistics.median(tails), 2),
                          "peak_host_bytes": peak}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=40)
    ap.add_argument("--chunk-mib", type=int, default=10)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--call-mib", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default=None, help="where the objects are written (default: the temp dir)")
    ap.add_argument("--side", choices=["buffered", "writer"], default=None)
    ap.add_argument("--sums", type=int, default=0, help="MXEC_SUM_* bits of the body digests both sides produce")
    a = ap.parse_args()
    if a.sums and a.side != "writer" and (not a.sums & 1 or a.sums & ~1 not in (0, 2, 4, 8, 16)):
        ap.error("the buffered side takes MD5 plus at most one checksum: --sums 1, 3, 5, 9 or 17")
    if a.side:
        side(a)
        return 0
    out = {}
    for s in ("buffered", "writer"):  # a fresh process each: its own peak
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", s, "--mib", str(a.mib),
                            "--chunk-mib", str(a.chunk_mib), "--m", str(a.m), "--call-mib", str(a.call_mib),
                            "--reps", str(a.reps), "--sums", str(a.sums)] + (["--dir", a.dir] if a.dir else []),
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line)
        out[s] = json.loads(line)
    print(json.dumps({"writer_over_buffered_wall": round(out["writer"]["wall_ms_median"] / out["buffered"]["wall_ms_median"], 3),
                      "writer_over_buffered_peak_host": round(out["writer"]["peak_host_bytes"] /
                                                              max(1, out["buffered"]["peak_host_bytes"]), 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
