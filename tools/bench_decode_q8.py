#!/usr/bin/env python3
"""Decode over an e4m3 cache, three calls on the same inputs, interleaved under graph replay (profiles/r11/README.md):
  A  fp8 queries under AUTO         (decode_splitkv_q8, library 0.12.0)
  B  bf16 queries                   (decode_splitkv_fp8)
  C  fp8 queries, MI355_SELECT_2D   (prefill_mfma_q8, what 0.11.0 did)
Usage: python tools/bench_decode_q8.py [--shapes B:KV:HQ:HK ...] [--segments 0 ...] [--rounds 7] [--per-graph 10]"""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vllm-triton-backend_amd")]
import torch  # noqa: E402

from mi355_attn import _lib  # noqa: E402
from mi355_attn.kernels import unified as ua_mod  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["16:32768:64:8", "64:8192:32:8", "1:8192:32:8", "1:32768:32:8"])
    ap.add_argument("--segments", type=int, nargs="*", default=[0], help="num_segments of call A (a sweep of its split count)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    dev, page, lib = torch.device("cuda:0"), 32, _lib.load()
    torch.manual_seed(0)
    for shape in args.shapes:
        B, kv, hq, hk = (int(x) for x in shape.split(":"))
        ppseq = (kv + page - 1) // page
        nb = B * ppseq + 8
        k = (torch.rand(nb, page, hk, 128, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        v = (torch.rand(nb, page, hk, 128, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        qb = (torch.rand(B, hq, 128, device=dev) * 2 - 1).to(torch.bfloat16)
        q8 = qb.to(torch.float8_e4m3fn)
        bt = torch.randperm(nb, device=dev)[: B * ppseq].to(torch.int32).view(B, ppseq)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev)
        sl = torch.full((B,), kv, dtype=torch.int32, device=dev)
        one = torch.ones(1, device=dev)
        algo_bytes = B * kv * hk * 128 * 2
        calls = [(f"A seg={s}", q8, None, s) for s in args.segments] + [("B", qb, None, 0), ("C", q8, 2, 0)]
        graphs, outs = [], []
        for label, q, force, seg in calls:
            out = torch.zeros(B, hq, 128, dtype=torch.bfloat16, device=dev)
            p, keep = ua_mod.fill_attn_params(q, k, v, out, cu, 1, sl, kv, 1.0 / math.sqrt(128), (-1, -1), bt, 0.0, one, one, None, force, num_segments=seg)
            nbytes = lib.mi355_attn_workspace_bytes(ctypes.byref(p))
            ws = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)      # the caller's own: nothing is allocated or cleared inside the capture

            def call(p=p, ws=ws, nbytes=nbytes):
                _lib.check(lib.mi355_unified_attention(ctypes.byref(p), ws.data_ptr(), nbytes, _lib.current_stream_handle(dev)), "bench")

            call()
            torch.cuda.synchronize()
            name = _lib.last_kernel()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.per_graph):
                    call()
            g.replay()
            torch.cuda.synchronize()
            graphs.append((label, name, g, (p, keep, ws)))
            outs.append(out)
        for (label, _, _, _), o in zip(graphs[:-2], outs[:-2]):      # A against C: the same arithmetic on another kernel
            print(f"{shape} {label}: max|A - C| {(o.float() - outs[-1].float()).abs().max().item():.3e}  max|A - B| {(o.float() - outs[-2].float()).abs().max().item():.3e}")
        times = {label: [] for label, _, _, _ in graphs}
        for _ in range(args.rounds):
            for label, _, g, _ in graphs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[label].append(e0.elapsed_time(e1) * 1e-3 / args.per_graph)
        for label, name, _, _ in graphs:
            ts = sorted(times[label])
            med = ts[len(ts) // 2]
            print(f"{shape} {label:9s} {name:20s} median {med * 1e6:8.1f} us  min {ts[0] * 1e6:8.1f}  max {ts[-1] * 1e6:8.1f}  "
                  f"{algo_bytes / med / 1e12:6.3f} TB/s  frac_of_8TB/s={algo_bytes / med / 8e12:5.3f}", flush=True)


if __name__ == "__main__":
    main()
