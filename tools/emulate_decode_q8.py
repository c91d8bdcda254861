"""CPU emulation of decode_q8_kernel's arithmetic (csrc/decode_q8.hip) on the inputs of tests/test_gpu_decode_q8.py, against the
float64 reference that test uses: 128-key tiles, a true running maximum, P = 2^8 exp(s - m) as two e4m3 terms, the row sum from
the rounded terms, fp32 accumulation, fp32 merge of the planned splits, bf16 output. Prints the largest absolute error per
configuration and overall (plain / peaked): the test's atol is twice that. One-off: python tools/emulate_decode_q8.py"""

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import paged_attention_oracle as orc  # noqa: E402

BF, E4, E5, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2, torch.float32
KV_LENS = [1, 127, 128, 129, 257, 777, 1500]
KS, VS, TILE = 0.0237, 0.041, 128


def e4m3(x):
    return x.to(E4).to(F32)


def plan(segments, num_seqs, hk):
    """plan_q8_splits: host-known sizes only."""
    max_tiles = (max(KV_LENS) + TILE - 1) // TILE
    want = segments if segments > 0 else min((1024 + num_seqs * hk - 1) // (num_seqs * hk), 32)
    want = max(1, min(want, max_tiles, 128))
    tps = (max_tiles + want - 1) // want
    return max(1, (max_tiles + tps - 1) // tps)


def row(q, K, V, c2, n, window, splits):
    """q [D], K / V [n, D] raw fp8 values in fp32 -> the normalised fp32 output row before v_scale."""
    lo_key = max(0, n - window) if window else 0
    t_lo, t_hi = lo_key // TILE, (n + TILE - 1) // TILE
    tps = max(1, (t_hi - t_lo + splits - 1) // splits)
    s_all = (K @ q).to(F32)
    parts = []
    for t0 in range(t_lo, t_hi, tps):
        m, l, o = -math.inf, torch.zeros((), dtype=F32), torch.zeros(128, dtype=F32)
        for t in range(t0, min(t0 + tps, t_hi)):
            a, b = max(t * TILE, lo_key), min((t + 1) * TILE, n)
            s = s_all[a:b]
            m_new = max(m, float(s.max()))
            alpha = torch.exp2(torch.tensor((m - m_new) * c2, dtype=F32)) if m > -math.inf else torch.ones((), dtype=F32)
            e = torch.exp2(s * c2 + torch.tensor(8.0 - m_new * c2, dtype=F32))
            hi = e4m3(e)
            pl = e4m3(e - hi)
            o = o * alpha + (hi @ V[a:b] + pl @ V[a:b])
            l = l * alpha + (hi.sum() + pl.sum())
            m = m_new
        parts.append((torch.tensor(m * c2, dtype=F32), l / 256, o / 256))
    m_all = max(p[0] for p in parts)
    w = [torch.exp2(p[0] - m_all) for p in parts]
    return sum(p[2] * wi for p, wi in zip(parts, w)) / sum(p[1] * wi for p, wi in zip(parts, w))


def emulate(kv_dtype, hq, hk, page, window, max_value, segments):
    inp = orc.make_paged_inputs(312, [1] * len(KV_LENS), KV_LENS, hq, hk, 128, page, BF, kv_dtype=kv_dtype, kv_scale=KS, max_value=max_value)
    q = inp["q"].to(E4).to(F32)
    ref = orc.dense_attention_fp64(q, inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"], inp["scale"],
                                   sliding_window=window, k_scale=KS, v_scale=VS)
    c2 = float(torch.tensor(inp["scale"], dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32) * torch.tensor(KS, dtype=F32))
    splits = plan(segments, len(KV_LENS), hk)
    out = torch.zeros(len(KV_LENS), hq, 128, dtype=F32)
    for i, n in enumerate(KV_LENS):
        pages = inp["block_table"][i, : (n + page - 1) // page].long()
        for h in range(hq):
            K = inp["k_cache"][pages, :, h // (hq // hk)].reshape(-1, 128)[:n].to(F32)
            V = inp["v_cache"][pages, :, h // (hq // hk)].reshape(-1, 128)[:n].to(F32)
            out[i, h] = row(q[i, h], K, V, c2, n, window, splits) * torch.tensor(VS, dtype=F32)
    return float((out.to(BF).double() - ref).abs().max())


if __name__ == "__main__":
    shapes = [(kv, *c) for kv in (E4, E5) for c in ((8, 2, 32), (6, 2, 32), (16, 1, 128))]
    plain = [(*s, 0, 1.0, seg) for s in shapes for seg in (1, 3, 8)] + [(E4, 8, 2, 32, w, 1.0, 3) for w in (8, 128, 200)]
    plain += [(E4, 8, 2, 32, 0, 1.0, 0), (E4, 32, 1, 32, 0, 1.0, 1)]
    peaked = [(E4, 8, 2, 32, 0, 3.0, seg) for seg in (1, 3, 8)]
    for label, cfgs in (("plain", plain), ("peaked", peaked)):
        worst = 0.0
        for cfg in cfgs:
            err = emulate(*cfg)
            worst = max(worst, err)
            print(f"{label} {cfg}: max|err| {err:.3e}", flush=True)
        print(f"{label}: largest {worst:.3e} -> atol {2 * worst:.1e}")
