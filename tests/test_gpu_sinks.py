"""-m gpu: attention sinks (`sinks=`, library 0.7.0) through every kernel family, against a plain float64 computation of
    out = sum_j exp(x_j) v_j / (exp(sink) + sum_j exp(x_j)),   lse = log(exp(sink) + sum_j exp(x_j))
written out below. Key and query lengths are chosen against the dispatch thresholds of csrc/ (plan_splits / plan_merge,
plan_key_splits, prefill_pw_selected, prefill_lat_selected); every case also checks that the call runs on the kernel it
runs on without sinks."""

import math
import types

import pytest
import torch

import golden_io
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu

FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def reference(t, scale, sinks, *, window=0, softcap=0.0, kv_scale=1.0):
    """float64 on the device: per sequence, gather its pages, one dense softmax per head with the sink as one more column."""
    q, kc, vc = t["q"], t["k_cache"], t["v_cache"]
    (T, Hq, D), page, Hk = q.shape, kc.shape[1], kc.shape[2]
    out = torch.zeros(T, Hq, D, dtype=torch.float64, device=q.device)
    lse = torch.zeros(T, Hq, dtype=torch.float64, device=q.device)
    cu, sk = t["cu_seqlens_q"].tolist(), t["seqused_k"].tolist()
    for i, n in enumerate(sk):
        q0, q1 = cu[i], cu[i + 1]
        ctx = n - (q1 - q0)
        pages = t["block_table"][i, : (n + page - 1) // page].long()

        def rows(c):                                        # [Hq, n, D]; fp8: (fp8 -> f32) * scale -> query type
            x = c[pages].reshape(-1, Hk, D)[:n]
            x = (x.float() * kv_scale).to(q.dtype) if c.dtype in FP8 else x
            return x.double().permute(1, 0, 2).repeat_interleave(Hq // Hk, 0)

        S = scale * torch.einsum("thd,hnd->htn", q[q0:q1].double(), rows(kc))
        if softcap:
            S = softcap * torch.tanh(S / softcap)
        qp, kp = torch.arange(q1 - q0, device=q.device)[:, None] + ctx, torch.arange(n, device=q.device)[None, :]
        if t.get("alibi_slopes") is not None:
            S = S + t["alibi_slopes"].double()[:, None, None] * (kp - ctx)
        mask = kp <= qp
        if window:
            mask = mask & (qp - kp < window)
        S = torch.cat([S.masked_fill(~mask, -math.inf), sinks.double()[:, None, None].expand(Hq, q1 - q0, 1)], -1)
        l = torch.logsumexp(S, -1)
        out[q0:q1] = torch.einsum("htn,hnd->thd", torch.exp(S - l[..., None])[..., :n], rows(vc))
        lse[q0:q1] = l.T
    return out, lse


def run(t, scale, sinks, *, window=0, softcap=0.0, kv_scale=None):
    from mi355_attn import _lib
    from mi355_attn.kernels import unified_attention_with_sinks

    q = t["q"]
    out = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:2], float("nan"), dtype=torch.float32, device=q.device)
    ql = t["cu_seqlens_q"][1:] - t["cu_seqlens_q"][:-1]
    ks = None if kv_scale is None else torch.tensor([kv_scale], dtype=torch.float32, device=q.device)
    unified_attention_with_sinks(
        q=q, k=t["k_cache"], v=t["v_cache"], out=out, cu_seqlens_q=t["cu_seqlens_q"], max_seqlen_q=int(ql.max()), seqused_k=t["seqused_k"],
        max_seqlen_k=int(t["seqused_k"].max()), avg_seqlen_q=0, avg_seqlen_k=0, softmax_scale=scale, causal=True,
        window_size=(window - 1, 0) if window else (-1, -1), block_table=t["block_table"], softcap=softcap, q_descale=None, k_descale=ks, v_descale=ks,
        alibi_slopes=t.get("alibi_slopes"), softmax_lse=lse, sinks=sinks)
    torch.cuda.synchronize()
    return out, lse, _lib.last_kernel()


BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# name: (query lens, key lens, Hq, Hk, D, dtype, expected kernel, options)
#   sinks: "ramp" (default; one value per head over [-8, 8]: no two heads of a KV group share one), "zero", 40.0, -inf
#   low: every score of the FIRST sequence lies below -150 (q = +4, k = -4 in every dimension: -16 D scale = -181 at D 128)
CASES = {
    "01_decode_single_gptoss": ([1] * 3, [20, 5, 32], 64, 8, 64, BF, "decode_single", {}),
    "02_decode_single_d128_f16": ([1] * 3, [20, 5, 32], 32, 8, 128, F16, "decode_single", {}),
    # batch 1, G 4, D 128: up to 8 splits merge in the kernel (plan_merge: one_trip = 16 / 4 * 2); 250 keys = 8 tiles
    "03_decode_flat_merge": ([1], [250], 8, 2, 128, BF, "decode_splitkv", {"ws_above": 256 << 10}),
    # 600 keys = 19 splits: more than one trip, not above 32 -> reduce_splits_kernel
    "04a_decode_reduce_kernel": ([1], [600], 8, 2, 128, BF, "decode_splitkv", {}),
    # 2100 keys = 66 splits on 4 waves' worth of rows -> the two-level merge; the 40-key row ends in its first workgroup
    "04b_decode_two_level_merge": ([1, 1], [2100, 40], 8, 2, 128, BF, "decode_splitkv", {}),
    # G 8, 4 tokens: two column groups; 32 splits -> reduce_splits_kernel over (unit, token) rows / one split / two, merged in the kernel
    "05a_decode_packed_reduce": ([4] * 3, [300, 37, 1000], 16, 2, 128, BF, "decode_splitkv_pack2", {}),
    "05b_decode_packed_single": ([4] * 3, [20, 30, 9], 16, 2, 128, BF, "decode_single_pack2", {}),
    "05c_decode_packed_flat": ([4] * 3, [64, 40, 50], 16, 2, 128, BF, "decode_splitkv_pack2", {}),
    "06_decode_window_d64": ([1] * 3, [700, 33, 300], 64, 8, 64, BF, "decode_splitkv", {"window": 128}),
    "07_decode_fp8": ([1] * 4, [700, 33, 300, 17], 8, 2, 128, F16, "decode_splitkv_fp8", {"kv": torch.float8_e4m3fn}),
    "08_prefill_short": ([200], [200], 8, 2, 128, BF, "prefill_mfma_lat", {}),
    "09_prefill_pw": ([2100], [2100], 32, 8, 128, BF, "prefill_mfma_pw", {}),
    "10_prefill_pw_d64": ([2100], [2100], 64, 8, 64, BF, "prefill_mfma_pw", {}),
    "11_prefill_pw_f16_late_rise": ([2100], [2100], 32, 8, 128, F16, "prefill_mfma_pw", {"needle": (1500, 5)}),
    "12_prefill_pw_fp8": ([2100], [2100], 32, 8, 128, BF, "prefill_mfma_pw_fp8", {"kv": torch.float8_e4m3fn}),
    "13_prefill_window_d64": ([300], [300], 64, 8, 64, BF, "prefill_mfma_feat", {"window": 128}),
    "14a_prefill_softcap": ([600], [600], 8, 2, 128, BF, "prefill_mfma_pw_sc", {"softcap": 30.0}),
    "14b_prefill_softcap_staged": ([300], [300], 8, 2, 128, BF, "prefill_mfma_feat", {"softcap": 30.0}),
    "14c_prefill_alibi": ([600], [600], 8, 2, 128, BF, "prefill_mfma_pw_al", {"alibi": True}),
    # 64 tokens against 4200 / 2100 keys: two wide key splits on the 64-rows-per-wave kernel / four on the 4-wave LDS-DMA kernel
    "15a_prefill_ksplit_pw": ([64], [4200], 8, 2, 128, BF, "prefill_mfma_pw_ksplit", {}),
    "15b_prefill_ksplit_dma": ([64], [2100], 8, 2, 128, BF, "prefill_mfma_ksplit", {}),
    "16_mixed_step": ([1, 200, 1, 300, 1], [900, 200, 17, 333, 33], 8, 2, 128, BF, "prefill_mfma_lat+decode_splitkv_pack", {}),
    "17_decode_scores_far_below_sink": ([1] * 3, [20, 5, 32], 32, 8, 128, F16, "decode_single", {"sinks": "zero", "low": True}),
    "18_prefill_scores_far_below_sink": ([2100], [2100], 32, 8, 128, BF, "prefill_mfma_pw", {"sinks": "zero", "low": True}),
    "19a_decode_sinks_plus_40": ([1] * 3, [20, 5, 32], 64, 8, 64, BF, "decode_single", {"sinks": 40.0}),
    "19b_prefill_sinks_plus_40": ([2100], [2100], 32, 8, 128, BF, "prefill_mfma_pw", {"sinks": 40.0}),
    "20a_decode_sinks_minus_inf": ([1], [250], 8, 2, 128, BF, "decode_splitkv", {"sinks": -math.inf}),
    "20b_prefill_sinks_minus_inf": ([2100], [2100], 32, 8, 128, BF, "prefill_mfma_pw", {"sinks": -math.inf}),
    "21_generic_f32_odd_head_size": ([1, 40, 9], [70, 45, 33], 6, 2, 40, F32, "generic", {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_sinks_in_every_kernel_family(name):
    import ctypes

    import gpu_util
    from mi355_attn import _lib
    from mi355_attn.kernels import unified

    q_lens, kv_lens, hq, hk, d, dtype, expect, opt = CASES[name]
    kv_dtype, kv_scale = opt.get("kv"), (0.5 if opt.get("kv") else None)
    inp = orc.make_paged_inputs(90, q_lens, kv_lens, hq, hk, d, 16, dtype, **(dict(kv_dtype=kv_dtype, kv_scale=kv_scale) if kv_dtype else {}))
    if opt.get("low"):
        n_pages = (kv_lens[0] + 15) // 16
        inp["q"][: q_lens[0]] = 4.0
        inp["k_cache"][inp["block_table"][0, :n_pages].long()] = -4.0
    if opt.get("needle"):         # one row's score on key 64 lies +30 above the rest: past the keys an f16 row's reference comes from
        row, head = opt["needle"]
        direction = torch.nn.functional.normalize(torch.randn(d, generator=torch.Generator().manual_seed(91)), dim=0)
        inp["k_cache"][int(inp["block_table"][0, 4]), 0, head // (hq // hk)] = (direction * 8.0).to(dtype)
        inp["q"][row, head] = (inp["q"][row, head].float() * 0.25 + direction * (30.0 / inp["scale"] / 8.0)).to(dtype)
    t = gpu_util.to_dev(inp)
    if opt.get("alibi"):
        t["alibi_slopes"] = torch.tensor([2.0 ** -(i + 1) for i in range(hq)], dtype=torch.float32, device=gpu_util.DEV)
    s = opt.get("sinks", "ramp")
    sinks = torch.linspace(-8.0, 8.0, hq) if s == "ramp" else torch.zeros(hq) if s == "zero" else torch.full((hq,), s)
    sinks = sinks[torch.randperm(hq, generator=torch.Generator().manual_seed(92))].to(gpu_util.DEV)
    kw = dict(window=opt.get("window", 0), softcap=opt.get("softcap", 0.0))

    out, lse, kernel = run(t, inp["scale"], sinks, kv_scale=kv_scale, **kw)
    out0, lse0, kernel0 = run(t, inp["scale"], None, kv_scale=kv_scale, **kw)
    assert kernel == kernel0, (kernel, kernel0)
    if "ws_above" in opt:
        p, _keep = unified.fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], max(q_lens), t["seqused_k"], max(kv_lens), inp["scale"],
                                            None, t["block_table"], 0.0, None, None, None, None, sinks=sinks)
        assert _lib.load().mi355_attn_workspace_bytes(ctypes.byref(p)) > opt["ws_above"]

    ref, ref_lse = reference(t, inp["scale"], sinks, kv_scale=kv_scale or 1.0, **kw)
    atol, rtol = golden_io.tolerance(dtype, kv_dtype)
    lse_atol = 2e-2 if kv_dtype is None else 4e-2              # tests/test_gpu_lse.py
    err, lse_err = (out.double() - ref).abs().max().item(), (lse.double() - ref_lse).abs().max().item()
    print(f"{name}: kernel={kernel} max|out err|={err:.3e} max|lse err|={lse_err:.3e}")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    torch.testing.assert_close(out.double(), ref, atol=atol, rtol=rtol)
    torch.testing.assert_close(lse.double(), ref_lse, atol=lse_atol, rtol=0)
    rows0 = slice(0, q_lens[0])
    if opt.get("low"):            # nothing but the sink: out ~ 0, lse ~ 0
        assert out[rows0].abs().max().item() <= atol and lse[rows0].abs().max().item() <= lse_atol
    if s == 40.0:
        assert out.abs().max().item() <= atol and (lse - 40.0).abs().max().item() <= lse_atol
    if s == -math.inf:            # no sink at all: the sink-free call's result
        torch.testing.assert_close(out.float(), out0.float(), atol=atol, rtol=rtol)
        torch.testing.assert_close(lse, lse0, atol=lse_atol, rtol=0)
    assert kernel == expect, (kernel, expect)     # the case reached the path it was sized for


def test_backend_layer_with_sinks_prefill_then_decode():
    """MI355AttentionImpl(..., sinks=...) at the gpt-oss shape (Hq 64 / Hk 8 / D 64): a 300-token prefill step, then a decode
    step. The layer takes the two calls - the cache holds what a separate reshape_and_cache_flash stores - and the output is
    the reference's."""
    import gpu_util
    from mi355_attn.backend import attn
    from mi355_attn.kernels import reshape_and_cache_flash

    dev, dtype, hq, hk, d, page = gpu_util.DEV, torch.bfloat16, 64, 8, 64, 16
    sinks = torch.linspace(-8.0, 8.0, hq).to(dtype)                  # as vLLM hands it over: a parameter in the model's type
    impl = attn.MI355AttentionImpl(hq, d, 1.0 / math.sqrt(d), hk, None, None, "auto", sinks=sinks)
    layer = types.SimpleNamespace(_k_scale=torch.ones((), device=dev), _v_scale=torch.ones((), device=dev), _q_scale=torch.ones((), device=dev), _q_scale_float=1.0)
    for q_len, kv_len in ((300, 300), (1, 301)):
        inp = orc.make_paged_inputs(93 + q_len, [q_len], [kv_len], hq, hk, d, page, dtype)
        g = torch.Generator().manual_seed(94)
        k_new, v_new = (torch.rand(q_len, hk, d, generator=g) * 2 - 1).to(dtype), (torch.rand(q_len, hk, d, generator=g) * 2 - 1).to(dtype)
        pos = torch.arange(kv_len - q_len, kv_len)
        slots = (inp["block_table"][0, pos // page].long() * page + pos % page).to(dev)
        t = gpu_util.to_dev(inp)
        kv_cache = torch.stack([t["k_cache"], t["v_cache"]]).contiguous()
        kc_ref, vc_ref = t["k_cache"].clone(), t["v_cache"].clone()
        reshape_and_cache_flash(k_new.to(dev), v_new.to(dev), kc_ref, vc_ref, slots, "auto", None, None)
        md = attn.MI355AttentionMetadata(num_actual_tokens=q_len, max_query_len=q_len, avg_query_len=q_len, avg_seq_len=kv_len, query_start_loc=t["cu_seqlens_q"],
                                         max_seq_len=kv_len, seq_lens=t["seqused_k"], block_table=t["block_table"], slot_mapping=slots, use_cascade=False,
                                         common_prefix_len=0, cu_prefix_query_lens=None, prefix_kv_lens=None, suffix_kv_lens=None)
        out = torch.full((q_len, hq * d), float("nan"), dtype=dtype, device=dev)
        impl.forward(layer, t["q"], k_new.to(dev), v_new.to(dev), kv_cache, md, output=out)
        torch.cuda.synchronize()
        assert torch.equal(kv_cache[0].view(torch.int16), kc_ref.view(torch.int16)) and torch.equal(kv_cache[1].view(torch.int16), vc_ref.view(torch.int16))
        ref, _ = reference(dict(t, k_cache=kc_ref, v_cache=vc_ref), inp["scale"], sinks.float().to(dev))
        torch.testing.assert_close(out.view(q_len, hq, d).double(), ref, atol=2e-2, rtol=2e-2)
