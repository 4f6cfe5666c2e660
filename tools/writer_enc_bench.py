"""The streaming encrypted writer against the buffered encrypted PUT, and the
GCM kernel's window form against its contiguous form.

--kernel: device time (HIP events on one stream, median of --reps after two
untimed launches) of mxec_frames_encrypt_device into one contiguous run and of
mxec_frames_encrypt_window_device into a ring of chunk slots, over the same
16 and 1 024 plaintext frames of 64 KiB, with chunk_size 10 MiB (almost no
frame is cut) and 20 000 (every frame is cut three or four times).  Both
entry points prepare the key and upload their tables per call, inside the
timed span.

Otherwise: --threads bodies of --mib MiB in page-locked memory, each written
by its own thread, either by mxec_put_object_chunked_encrypted in one call
(--side buffered) or through mxec_writer_open_encrypted in --call-mib pieces
(--side writer).  Each side runs in a fresh process, as tools/writer_bench.py
does: a small PUT first, the resident set noted, one round of PUTs under a
sampler of the resident set (its peak less the note: the host bytes the
library took), then --reps timed rounds.  One JSON line per side and one with
the ratios.

    python tools/writer_enc_bench.py [--mib 40 --chunk-mib 10 --m 2 --threads 1 --reps 5]
    python tools/writer_enc_bench.py --kernel
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from writer_bench import PeakResident, resident  # noqa: E402

KEY, PREFIX, AAD = bytes(range(32)), b"\x80\x01\x02\x03", b"bucket\0key\0v\0"
FRAME = 65536


def kernel(a) -> None:
    import numpy as np
    import torch

    import maxio_amd

    with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        stream = torch.cuda.current_stream().cuda_stream
        for frames in (16, 1024):
            n, span = frames * FRAME, frames * (FRAME + 28)
            pt = torch.from_numpy(np.random.default_rng(2).integers(0, 256, n, dtype=np.uint8)).cuda()
            aad = torch.zeros(frames * 32, dtype=torch.uint8, device="cuda")
            job = {"key": KEY, "nonce_prefix": PREFIX, "frame_size": FRAME, "aad_dev": aad.data_ptr(), "aad_len": 32,
                   "in_dev": pt.data_ptr(), "len": n}

            def timed(fn):
                ms = []
                for r in range(a.reps + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if r >= 2:
                        ms.append(e0.elapsed_time(e1))
                return statistics.median(ms), min(ms)

            out = torch.empty(span, dtype=torch.uint8, device="cuda")
            flat = timed(lambda: ctx.frames_device([dict(job, out_dev=out.data_ptr())], stream=stream))
            row = {"frames": frames, "contiguous_ms_median": round(flat[0], 4), "contiguous_ms_min": round(flat[1], 4)}
            for c in (10 << 20, 20000):
                stride = (c + 255) // 256 * 256
                slots = (span + c - 1) // c + 1
                win = torch.empty(slots * stride, dtype=torch.uint8, device="cuda")
                w = timed(lambda: ctx.frames_encrypt_window_device(job, 12345, win.data_ptr(), c, stride, slots,
                                                                   stream=stream))
                row["window_c%d_ms_median" % c] = round(w[0], 4)
                row["window_c%d_ms_min" % c] = round(w[1], 4)
                row["window_c%d_over_contiguous" % c] = round(w[0] / flat[0], 3)
            print(json.dumps(row))


def side(a) -> None:
    import numpy as np

    import maxio_amd

    n, c, piece = a.mib << 20, a.chunk_mib << 20, a.call_mib << 20
    root = tempfile.mkdtemp(prefix="writer_enc_bench_", dir=a.dir)
    try:
        with maxio_amd.Context(device_mask=1, streams_per_device=max(2, min(a.threads, 16))) as ctx:
            body = ctx.host_array(n)
            body[:] = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)

            def put(d, n=n, c=c):
                if a.side == "buffered":
                    ctx.put_object_chunked_encrypted(d, c, a.m, KEY, PREFIX, AAD, body[:n])
                    return
                w = ctx.open_writer_encrypted(d, c, a.m, n, KEY, PREFIX, AAD)
                for o in range(0, n, piece):
                    w.write(body[o:min(n, o + piece)])
                w.finish()
                w.close()

            def round_(tag):
                errors = []

                def one(i):
                    try:
                        put(os.path.join(root, "%s_%d.ec" % (tag, i)))
                    except Exception as e:  # noqa: BLE001
                        errors.append(repr(e))

                ts = [threading.Thread(target=one, args=(i,)) for i in range(a.threads)]
                t0 = time.perf_counter()
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                wall = time.perf_counter() - t0
                assert not errors, errors
                shutil.rmtree(root, ignore_errors=True)
                os.makedirs(root, exist_ok=True)
                return wall

            put(os.path.join(root, "warm.ec"), n=4 << 16, c=1 << 16)
            before = resident()
            with PeakResident() as pr:
                round_("first")
            peak = pr.peak - before
            walls = [round_("r%d" % r) for r in range(a.reps)]
            ctx.host_free(body)
        print(json.dumps({"side": a.side, "threads": a.threads, "body_mib": a.mib, "chunk_mib": a.chunk_mib, "m": a.m,
                          "call_mib": a.call_mib, "wall_ms_median": round(1e3 * statistics.median(walls), 2),
                          "wall_ms_min": round(1e3 * min(walls), 2), "wall_ms": [round(1e3 * w, 2) for w in walls],
                          "peak_host_bytes": peak}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--mib", type=int, default=40)
    ap.add_argument("--chunk-mib", type=int, default=10)
    ap.add_argument("--m", type=int, default=2)
    ap.add_argument("--call-mib", type=int, default=1)
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the objects are written (default: the temp dir)")
    ap.add_argument("--side", choices=["buffered", "writer"], default=None)
    a = ap.parse_args()
    if a.kernel:
        kernel(a)
        return 0
    if a.side:
        side(a)
        return 0
    out = {}
    for s in ("buffered", "writer"):  # a fresh process each: its own peak
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", s, "--mib", str(a.mib),
                            "--chunk-mib", str(a.chunk_mib), "--m", str(a.m), "--call-mib", str(a.call_mib),
                            "--threads", str(a.threads), "--reps", str(a.reps)] + (["--dir", a.dir] if a.dir else []),
                           capture_output=True, text=True, timeout=400)
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
