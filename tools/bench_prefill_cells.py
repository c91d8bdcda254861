#!/usr/bin/env python3
"""Chunked-prefill cells at one head geometry in ONE process (tools/bench_prefill.py measures one shape per process): for every
cell (sequences x chunk tokens over total keys), cache type, window and forced split count, 20 launches in a HIP graph, replayed
untimed for 0.25 s and then `--replays` times under an event pair each. One JSON line per measurement: median / min / max us
per launch and the kernel name. MI355_LIB=<path> measures another build of the library (the A/B of profiles/r12/)."""
import argparse
import json
import math
import os
import time

os.environ.setdefault("MI355_LAB", "1")
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vllm-triton-backend_amd")]
import torch  # noqa: E402

from mi355_attn import _lib  # noqa: E402
from mi355_attn.kernels import unified as ua_mod  # noqa: E402

LAUNCHES = 20


def measure(dev, batch, chunk, keys, hq, hk, d, kvdtype, window, segments, replays, page=16):
    dt = torch.bfloat16
    kvdt = torch.float8_e4m3fn if kvdtype == "fp8" else dt
    pps = (keys + page - 1) // page
    nb = int(batch * pps * 1.25)
    g = torch.Generator(device=dev).manual_seed(0)
    k = (torch.rand(nb, page, hk, d, device=dev, generator=g) * 2 - 1).to(kvdt)
    v = (torch.rand(nb, page, hk, d, device=dev, generator=g) * 2 - 1).to(kvdt)
    q = (torch.rand(batch * chunk, hq, d, device=dev, generator=g) * 2 - 1).to(dt)
    ksc = torch.ones(1, device=dev) if kvdt != dt else None
    bt = torch.randperm(nb, device=dev, generator=g)[: batch * pps].to(torch.int32).view(batch, pps)
    cu = (torch.arange(batch + 1, dtype=torch.int32, device=dev) * chunk).to(torch.int32)
    sl = torch.full((batch,), keys, dtype=torch.int32, device=dev)
    out = torch.empty_like(q)
    p, keep = ua_mod.fill_attn_params(q, k, v, out, cu, chunk, sl, keys, 1.0 / math.sqrt(d), (window - 1, 0) if window else (-1, -1), bt, 0.0,
                                      ksc, ksc, None, None, num_segments=segments)
    torch.cuda.synchronize()         # the inputs were written on the default stream, the launches below run on another one
    gs, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    ts = []
    with torch.cuda.stream(gs):
        ua_mod.launch(p, dev)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=gs):
            for _ in range(LAUNCHES):
                ua_mod.launch(p, dev)
        t_end = time.perf_counter() + 0.25                   # clock / power ramp, untimed
        while time.perf_counter() < t_end:
            graph.replay()
            torch.cuda.synchronize()
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(gs)
            graph.replay()
            e1.record(gs)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    ts.sort()
    return {"batch": batch, "chunk": chunk, "keys": keys, "kv": kvdtype, "window": window, "segments": segments, "kernel": _lib.last_kernel(),
            "us_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2), "mean_abs_out": float(out.float().abs().mean())}


def main():
    if os.environ.get("MI355_LIB"):
        _lib.LIB_PATH = os.path.abspath(os.environ["MI355_LIB"])
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1x512@8192,1x512@32768,1x2048@8192,1x2048@32768,1x2048@2048,1x4096@4096,16x4096@4096",
                    help="comma-separated <sequences>x<chunk tokens>@<keys per sequence>")
    ap.add_argument("--variants", default="same:0,fp8:0,same:1024", help="comma-separated <same|fp8>:<window>")
    ap.add_argument("--segments", default="0", help="comma-separated num_segments values (0 = the library's plan, 1 = no key split)")
    ap.add_argument("--hq", type=int, default=16)
    ap.add_argument("--hk", type=int, default=8)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--replays", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sink = open(args.out, "a") if args.out else None
    for variant in args.variants.split(","):
        kvdtype, window = variant.split(":")
        for cell in args.cells.split(","):
            shape, keys = cell.split("@")
            batch, chunk = shape.split("x")
            for s in args.segments.split(","):
                r = dict(measure(dev, int(batch), int(chunk), int(keys), args.hq, args.hk, args.d, kvdtype, int(window), int(s), args.replays), tag=args.tag)
                line = json.dumps(r)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()


if __name__ == "__main__":
    main()
