#!/usr/bin/env python3
"""locate_bench — mxec_locate beside the verify it shares its walk with, and
one-object heals from files.  Prints one JSON line.

(a) Clean stripes (per shape, one process, the same mxec_batch_alloc
buffers): after the encode has produced the parity and its grid tuner has
settled, mxec_verify_strided_device and mxec_locate_strided_device are
launched alternately, each timed by HIP events.  Both read (k + m) * S bytes
per object and write nothing.  The yardstick is the verify; the figure is
the ratio of the medians beside the verify's own run-to-run spread.

(b) One shard of every object overwritten with random bytes -- every wave
of every tile takes the classification path, the slow path's worst case --
once a data shard, once a parity shard; time as a multiple of (a).

  4+2x10M   4 + 2, 10 MiB shards,  256 objects
  4+2x1M    4 + 2,  1 MiB shards, 2048 objects
  8+4x10M   8 + 4, 10 MiB shards,  128 objects
  8+4x1M    8 + 4,  1 MiB shards, 1024 objects

(c) Lone object: one 4 + 2 x 10 MiB object written with put_object_chunked
(files in the page cache), one byte of one shard flipped before every call;
mxec_locate_object with HEAL and mxec_scrub_object with HEAL alternately,
wall time per call, and the SHA-256 messages each hashed.  Also the two ways
of naming the shard without healing: mxec_locate_object and the scrub's
DIGESTS mode.

Every GPU step runs in a child process under its own timeout; a step that
fails or runs out of time ends the run (nothing more is started on the GPU)
and is reported as such.

  python tools/locate_bench.py [--reps 10] [--objects-scale 1.0] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"4+2x10M": (4, 2, 10 << 20, 256), "4+2x1M": (4, 2, 1 << 20, 2048),
          "8+4x10M": (8, 4, 10 << 20, 128), "8+4x1M": (8, 4, 1 << 20, 1024)}
STEP_TIMEOUT_S = 240
VERIFY_OK = (1 << 64) - 1


class _DevMem:
    """A device allocation of the library as a torch-importable array."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}


def _stats(ms: list[float]) -> dict:
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 3), "n": len(ms)}


def kernel_step(name: str, reps: int, scale: float) -> dict:
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import maxio_amd

    k, m, S, n = SHAPES[name]
    n = max(8, int(n * scale))
    dev = torch.device("cuda:0")
    rec = np.dtype([("first_bad", "<u8"), ("n_bad", "<u8"), ("shard_min", "<u4"), ("shard_max", "<u4")])
    with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        ptr, stride, _ = ctx.batch_alloc(k, m, S, n)
        try:
            t = torch.as_tensor(_DevMem(ptr, n * (k + m) * stride), device=dev).view(n, k + m, stride)
            g = torch.Generator(device=dev).manual_seed(0x10CA)
            for o in range(n):  # per object keeps the randint temporary small
                t[o, :k, :S].copy_(torch.randint(0, 256, (k, S), dtype=torch.uint8, device=dev, generator=g))
            fb = torch.zeros(n * m, dtype=torch.int64, device=dev)
            out = torch.zeros(n * rec.itemsize, dtype=torch.uint8, device=dev)
            st = torch.cuda.Stream()
            ostride = (k + m) * stride
            data, parity = ptr, ptr + k * stride

            def encode():
                ctx.encode_strided_device(k, m, S, n, data, ostride, stride, parity, ostride, stride,
                                          stream=st.cuda_stream)

            def verify():
                ctx.verify_strided_device(k, m, S, n, data, ostride, stride, parity, ostride, stride,
                                          fb.data_ptr(), stream=st.cuda_stream)

            def locate():
                ctx.locate_strided_device(k, m, S, n, data, ostride, stride, parity, ostride, stride,
                                          out.data_ptr(), stream=st.cuda_stream)

            def records():
                return np.frombuffer(out.cpu().numpy().tobytes(), rec)

            def timed(fn) -> float:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                fn()
                b.record(st)
                b.synchronize()
                return a.elapsed_time(b)

            torch.cuda.synchronize()
            for _ in range(10):  # cold launch, then the tuner's trials (two per grid)
                encode()
                st.synchronize()
            for _ in range(3):
                verify()
                locate()
            st.synchronize()
            grid = ctx.rs_grid(k, m, S)
            ver, loc = [], []
            for _ in range(reps):  # alternating: both see the same minutes of the machine
                ver.append(timed(verify))
                loc.append(timed(locate))
            r = records()
            clean = bool((fb.cpu().numpy().view(np.uint64) == VERIFY_OK).all() and (r["n_bad"] == 0).all() and
                         (r["first_bad"] == VERIFY_OK).all())
            # (b) one shard of every object overwritten: a data shard, then (the
            # data restored by the XOR's inverse being itself) a parity shard.
            worst = {}
            for label, shard in (("data_shard", 1 % k), ("parity_shard", k + m - 1)):
                noise = torch.randint(1, 256, (S,), dtype=torch.uint8, device=dev, generator=g)  # every byte changes
                t[:, shard, :S] ^= noise
                torch.cuda.synchronize()
                locate()
                st.synchronize()
                ms = [timed(locate) for _ in range(reps)]
                r = records()
                named = bool((r["shard_min"] == shard).all() and (r["shard_max"] == shard).all() and
                             (r["n_bad"] == S).all() and (r["first_bad"] == 0).all())
                t[:, shard, :S] ^= noise
                torch.cuda.synchronize()
                worst[label] = dict(_stats(ms), every_object_named_exactly=named)
            locate()
            st.synchronize()
            restored = bool((records()["n_bad"] == 0).all())
        finally:
            torch.cuda.synchronize()
            ctx.batch_free(ptr)
    gb = n * (k + m) * S / 1e9
    v, l = _stats(ver), _stats(loc)
    v["GBps"], l["GBps"] = round(gb / v["median_ms"] * 1e3, 1), round(gb / l["median_ms"] * 1e3, 1)
    slower = 100.0 * (l["median_ms"] - v["median_ms"]) / v["median_ms"]
    for w in worst.values():
        w["times_clean_locate"] = round(w["median_ms"] / l["median_ms"], 2)
    return {"k": k, "m": m, "shard_size": S, "objects": n, "bytes_read_GB": round(gb, 3), "shard_stride": stride,
            "grid_blocks_per_cu": grid, "verify": v, "locate": l,
            "locate_over_verify": round(l["median_ms"] / v["median_ms"], 4),
            "locate_slower_than_verify_pct": round(slower, 3),
            "within_verify_spread": bool(slower <= v["spread_pct"]),
            "clean_batch_all_clean": clean, "one_shard_corrupt": worst, "clean_again_after": restored}


def object_step(reps: int) -> dict:
    import numpy as np

    sys.path.insert(0, ROOT)
    import maxio_amd

    chunk, k, m = 10 << 20, 4, 2
    body = np.random.default_rng(0x10CA).integers(0, 256, k * chunk, dtype=np.uint8)
    out = {"k": k, "m": m, "chunk_size": chunk, "files": "page cache", "damage": "one byte of shard 1 flipped"}
    with tempfile.TemporaryDirectory() as d, maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        ec = os.path.join(d, "obj.ec")
        os.makedirs(ec)
        ctx.put_object_chunked(ec, chunk, m, body)
        shard = os.path.join(ec, "000001")

        def flip():
            with open(shard, "r+b") as f:
                f.seek(chunk // 2)
                b = f.read(1)
                f.seek(chunk // 2)
                f.write(bytes([b[0] ^ 0x10]))

        def hashed():
            return ctx.combiner_stats(0)["messages"]

        def locate_heal():
            r = ctx.locate_object(ec, heal=True)
            assert (r["outcome"], r["shard"], r["healed"]) == (1, 1, 1), r

        def scrub_heal():
            r = ctx.scrub_object(ec, parity=True, heal=True)
            assert r["verdict"] == 2 and r["n_healed"] == 1, r

        def locate_name():
            r = ctx.locate_object(ec)
            assert (r["outcome"], r["shard"]) == (1, 1), r

        def scrub_name():
            r = ctx.scrub_object(ec, parity=False, digests=True)
            assert r["verdict"] == 1 and r["shard_state"][1] == 3, r

        times = {"locate_heal": [], "scrub_heal": [], "locate_name": [], "scrub_digests_name": []}
        msgs = {}
        for rep in range(reps + 1):  # the first round warms staging buffers and code objects
            # Damaged once for the two naming calls and the first heal, again for the second heal.
            for label, fn, damage in (("locate_name", locate_name, True), ("scrub_digests_name", scrub_name, False),
                                      ("locate_heal", locate_heal, False), ("scrub_heal", scrub_heal, True)):
                if damage:
                    flip()
                h0 = hashed()
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                msgs[label] = hashed() - h0
                if rep:
                    times[label].append(dt)
        for label, ms in times.items():
            out[label] = dict(_stats(ms), sha256_messages=msgs[label])
        assert ctx.get_object_chunked(ec) == body.tobytes()
    out["scrub_heal_over_locate_heal"] = round(out["scrub_heal"]["median_ms"] / out["locate_heal"]["median_ms"], 2)
    out["scrub_digests_over_locate_name"] = round(out["scrub_digests_name"]["median_ms"] /
                                                  out["locate_name"]["median_ms"], 2)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--objects-scale", type=float, default=1.0, help="fraction of each shape's object count")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        r = object_step(a.reps) if a.child == "object" else kernel_step(a.child, a.reps, a.objects_scale)
        print("RESULT " + json.dumps(r))
        return 0
    result = {"tool": "locate_bench", "reps": a.reps}
    for step in list(SHAPES) + ["object"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps),
               "--objects-scale", str(a.objects_scale)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"timed out after {STEP_TIMEOUT_S} s"}
            result["stopped_after"] = step
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            result[step] = {"error": f"exit {p.returncode}", "stderr": p.stderr[-800:]}
            result["stopped_after"] = step  # nothing more is started on the GPU
            break
        result[step] = json.loads(line[-1][len("RESULT "):])
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if "stopped_after" in result else 0


if __name__ == "__main__":
    sys.exit(main())
