#!/usr/bin/env python3
"""verify_bench — ReedSolomon::verify on the GPU beside the shipping encode,
and one-object scrubs from files.  Prints one JSON line.

Kernel rate (per shape, one process, the same mxec_batch_alloc buffers):
the encode and the verify are launched alternately, each timed by HIP events,
after both are warm and the encode's grid tuner has settled.  Both move
(k + m) * S bytes per object; the verify writes none.  The bar is the encode
on those buffers: the verify should not be slower than it by more than the
encode's own run-to-run spread, which the repeated timings give.

  cfg1  4 + 2, 10 MiB shards, 1024 objects   (BASELINE configs[1])
  ns    8 + 4,  1 MiB shards, 4096 objects   (the north-star shape)

Lone-object scrub: one 4 + 2 x 10 MiB object written with put_object_chunked
(files in the page cache), scrubbed in PARITY mode and in DIGESTS mode, wall
time per call.

Every GPU step runs in a child process under its own timeout; a step that
fails or runs out of time ends the run (nothing more is started on the GPU)
and is reported as such.

  python tools/verify_bench.py [--reps 10] [--objects-scale 1.0] [--out FILE]
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
SHAPES = {"cfg1": (4, 2, 10 << 20, 1024), "ns": (8, 4, 1 << 20, 4096)}
STEP_TIMEOUT_S = {"cfg1": 240, "ns": 240, "scrub": 180}
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
    with maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        ptr, stride, _ = ctx.batch_alloc(k, m, S, n)
        try:
            t = torch.as_tensor(_DevMem(ptr, n * (k + m) * stride), device=dev).view(n, k + m, stride)
            g = torch.Generator(device=dev).manual_seed(0x5C2B)
            for o in range(n):  # per object keeps the randint temporary small
                t[o, :k, :S].copy_(torch.randint(0, 256, (k, S), dtype=torch.uint8, device=dev, generator=g))
            fb = torch.zeros(n * m, dtype=torch.int64, device=dev)
            st = torch.cuda.Stream()
            ostride = (k + m) * stride
            data, parity = ptr, ptr + k * stride

            def encode():
                ctx.encode_strided_device(k, m, S, n, data, ostride, stride, parity, ostride, stride,
                                          stream=st.cuda_stream)

            def verify():
                ctx.verify_strided_device(k, m, S, n, data, ostride, stride, parity, ostride, stride,
                                          fb.data_ptr(), stream=st.cuda_stream)

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
            st.synchronize()
            grid = ctx.rs_grid(k, m, S)
            enc, ver = [], []
            for _ in range(reps):  # alternating: both see the same minutes of the machine
                enc.append(timed(encode))
                ver.append(timed(verify))
            res = fb.cpu().numpy().view(np.uint64)
            clean = bool((res == VERIFY_OK).all())
            # The timed size finds a flip too: last object, last row, last byte.
            t[n - 1, k + m - 1, S - 1] ^= 1
            torch.cuda.synchronize()
            verify()
            st.synchronize()
            res = fb.cpu().numpy().view(np.uint64).reshape(n, m)
            found = bool(res[n - 1, m - 1] == S - 1 and (res == VERIFY_OK).sum() == n * m - 1)
        finally:
            torch.cuda.synchronize()
            ctx.batch_free(ptr)
    gb = n * (k + m) * S / 1e9
    e, v = _stats(enc), _stats(ver)
    e["GBps"], v["GBps"] = round(gb / e["median_ms"] * 1e3, 1), round(gb / v["median_ms"] * 1e3, 1)
    slower = 100.0 * (v["median_ms"] - e["median_ms"]) / e["median_ms"]
    return {"k": k, "m": m, "shard_size": S, "objects": n, "bytes_moved_GB": round(gb, 3), "shard_stride": stride,
            "encode_grid_blocks_per_cu": grid, "encode": e, "verify": v,
            "verify_slower_than_encode_pct": round(slower, 3),
            "within_encode_spread": bool(slower <= e["spread_pct"]),
            "clean_batch_all_ok": clean, "flip_found_exactly": found}


def scrub_step(reps: int) -> dict:
    import numpy as np

    sys.path.insert(0, ROOT)
    import maxio_amd

    chunk, k, m = 10 << 20, 4, 2
    body = np.random.default_rng(0x5C2B).integers(0, 256, k * chunk, dtype=np.uint8)
    out = {"k": k, "m": m, "chunk_size": chunk, "files": "page cache"}
    with tempfile.TemporaryDirectory() as d, maxio_amd.Context(device_mask=1, streams_per_device=2) as ctx:
        ec = os.path.join(d, "obj.ec")
        os.makedirs(ec)
        ctx.put_object_chunked(ec, chunk, m, body)
        for label, mode in (("parity", dict(parity=True)), ("digests", dict(parity=False, digests=True))):
            r = ctx.scrub_object(ec, **mode)  # warm: staging buffers, code objects
            assert r["verdict"] == 0, r
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = ctx.scrub_object(ec, **mode)
                ms.append((time.perf_counter() - t0) * 1e3)
            assert r["verdict"] == 0, r
            out[label] = _stats(ms)
    out["digests_over_parity"] = round(out["digests"]["median_ms"] / out["parity"]["median_ms"], 2)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--objects-scale", type=float, default=1.0, help="fraction of each shape's object count")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        r = scrub_step(a.reps) if a.child == "scrub" else kernel_step(a.child, a.reps, a.objects_scale)
        print("RESULT " + json.dumps(r))
        return 0
    result = {"tool": "verify_bench", "reps": a.reps}
    for step in ("cfg1", "ns", "scrub"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(a.reps),
               "--objects-scale", str(a.objects_scale)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S[step])
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"timed out after {STEP_TIMEOUT_S[step]} s"}
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
