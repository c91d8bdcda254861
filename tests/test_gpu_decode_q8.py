"""-m gpu: decode_q8_kernel + decode_q8_merge_kernel (csrc/decode_q8.hip) - one e4m3 query token per sequence over an fp8 cache at
head size 128, bf16 output - against float64 dense attention on the dequantised inputs with the e4m3 query. One ragged batch: one
key; one under, on and over a 128-key tile; a ragged middle; 1500 keys (12 tiles: several splits).
Tolerance: rtol the project's bf16 2e-2; atol twice the largest error of a CPU emulation of the kernel's arithmetic
(tools/emulate_decode_q8.py: 128-key tiles, running maximum, two-term e4m3 P with the 2^8 factor, row sum from the rounded terms,
fp32 accumulation, fp32 merge of the planned splits, bf16 output) on exactly these inputs, over every configuration below:
emulated 3.9e-3 plain (window 8; 3.5e-3 without a window, the bf16 rounding of the one-key row), 1.485e-2 peaked -> atol 7.8e-3 /
2.97e-2."""

import ctypes
import functools

import pytest
import torch

import gpu_util
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu

BF, E4, E5 = torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2
KV_LENS = [1, 127, 128, 129, 257, 777, 1500]
KS, VS = 0.0237, 0.041
ATOL, ATOL_PEAKED, RTOL = 7.8e-3, 2.97e-2, 2e-2


@functools.lru_cache(maxsize=None)
def case(kv_dtype, hq, hk, page, window=0, max_value=1.0):
    """(inputs on the host with q in e4m3, float64 output, float64 lse) - computed once per configuration and shared."""
    inp = orc.make_paged_inputs(312, [1] * len(KV_LENS), KV_LENS, hq, hk, 128, page, BF, kv_dtype=kv_dtype, kv_scale=KS, max_value=max_value)
    inp["q"] = inp["q"].to(E4)
    ref, lse = orc.dense_attention_fp64(inp["q"].float(), inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                        inp["scale"], sliding_window=window, k_scale=KS, v_scale=VS, return_lse=True)
    return inp, ref, lse


def run(inp, segments, window=0, force=None, no_workspace=False, max_k=max(KV_LENS), **kw):
    """One call through the C ABI: (out, kernel, the workspace or None)."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified

    t = gpu_util.to_dev(inp)
    out = torch.full(t["q"].shape, float("nan"), dtype=BF, device=gpu_util.DEV)
    kst, vst = torch.tensor([KS], device=gpu_util.DEV), torch.tensor([VS], device=gpu_util.DEV)
    p, _keep = unified.fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], 1, t["seqused_k"], max_k, inp["scale"],
                                        (window - 1, 0) if window else None, t["block_table"], 0.0, kst, vst, None, force, num_segments=segments, **kw)
    lib = _lib.load()
    nbytes = lib.mi355_attn_workspace_bytes(ctypes.byref(p))
    ws = None if no_workspace or nbytes == 0 else torch.zeros(nbytes, dtype=torch.uint8, device=gpu_util.DEV)
    _lib.check(lib.mi355_unified_attention(ctypes.byref(p), _lib.ptr(ws), 0 if ws is None else nbytes, _lib.current_stream_handle(gpu_util.DEV)), "decode_q8")
    torch.cuda.synchronize()
    return out, _lib.last_kernel(), ws


def check(out, ref, atol=ATOL):
    assert not torch.isnan(out).any()
    print(f"max|err| {(out.double().cpu() - ref).abs().max():.3e} (atol {atol})")
    torch.testing.assert_close(out.double().cpu(), ref, atol=atol, rtol=RTOL)


def name(segments):
    return "decode_single_q8" if segments == 1 else "decode_splitkv_q8"


@pytest.mark.parametrize("segments", [1, 3, 8])
@pytest.mark.parametrize("kv_dtype,hq,hk,page,max_value", [(kv, *c, 1.0) for kv in (E4, E5) for c in ((8, 2, 32), (6, 2, 32), (16, 1, 128))] + [(E4, 8, 2, 32, 3.0)])
def test_plain_matches_float64(kv_dtype, hq, hk, page, max_value, segments):
    """Eight segments: the short sequences' trailing splits are empty, the long ones' count caps at their tiles. max_value 3.0: peaked."""
    inp, ref, _ = case(kv_dtype, hq, hk, page, max_value=max_value)
    out, kernel, _ = run(inp, segments)
    assert kernel == name(segments)
    check(out, ref, ATOL if max_value == 1.0 else ATOL_PEAKED)


@pytest.mark.parametrize("window", [8, 128, 200])
def test_sliding_window_matches_float64(window):
    """The window's first tile is not tile 0 for the long sequences: a row's splits start there."""
    inp, ref, _ = case(E4, 8, 2, 32, window)
    out, kernel, _ = run(inp, 3, window)
    assert kernel == "decode_splitkv_q8"
    check(out, ref)


@pytest.mark.parametrize("segments", [1, 3])
def test_sinks_and_lse(segments):
    """From the sink-free float64 result: lse = log(exp(lse0) + exp(sink)), out = out0 * exp(lse0 - lse)."""
    inp, out0, lse0 = case(E4, 8, 2, 32)
    sinks = torch.linspace(-2.0, 2.0, 8)[torch.randperm(8, generator=torch.Generator().manual_seed(313))]
    ref_lse = torch.logaddexp(lse0, sinks.double()[None, :])
    lse = torch.full(inp["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    out, kernel, _ = run(inp, segments, lse=lse, sinks=sinks.to(gpu_util.DEV))
    assert kernel == name(segments)
    check(out, out0 * torch.exp(lse0 - ref_lse)[..., None])
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double().cpu(), ref_lse, atol=2e-2, rtol=0)


def test_stale_nan_bytes_beyond_the_sequences_are_ignored():
    """0x7f is NaN in e4m3fn: every slot no sequence uses holds it, in both caches."""
    inp, ref, _ = case(E4, 8, 2, 32)
    inp = dict(inp, k_cache=inp["k_cache"].clone(), v_cache=inp["v_cache"].clone())
    used = torch.zeros(inp["k_cache"].shape[:2], dtype=torch.bool)
    for i, n in enumerate(KV_LENS):
        for j in range(n):
            used[inp["block_table"][i, j // 32], j % 32] = True
    for key in ("k_cache", "v_cache"):
        inp[key].view(torch.uint8)[~used] = 0x7F
    out, kernel, _ = run(inp, 3)
    assert kernel == "decode_splitkv_q8"
    check(out, ref)


def test_auto_plans_its_splits_and_leaves_the_counters_zero():
    """num_segments = 0 at max_seqlen_k = 1500: the library's own plan; the counter region at the head of its workspace stays zero."""
    inp, ref, _ = case(E4, 8, 2, 32)
    out, kernel, ws = run(inp, 0)
    assert kernel == "decode_splitkv_q8"
    check(out, ref)
    assert ws.numel() > (256 << 10) and not ws[: 256 << 10].any()


@pytest.mark.parametrize("segments", [0, 4])
def test_without_a_key_bound_one_split_walks_each_row_to_its_own_length(segments):
    """max_seqlen_k = 0, "none given": no plan can be made from it, whatever num_segments asks."""
    inp, ref, _ = case(E4, 8, 2, 32)
    out, kernel, ws = run(inp, segments, max_k=0)
    assert kernel == "decode_single_q8" and ws is None
    check(out, ref)


@pytest.mark.parametrize("how", ["select_2d", "group_32", "no_workspace"])
def test_what_stays_on_the_q_block_kernel(how):
    """MI355_SELECT_2D (the A/B handle), G = 32, and a multi-split plan called without its workspace (a 0.11.0 caller)."""
    inp, ref, _ = case(E4, 32, 1, 32) if how == "group_32" else case(E4, 8, 2, 32)
    out, kernel, _ = run(inp, 3 if how == "no_workspace" else 0, force=2 if how == "select_2d" else None, no_workspace=how == "no_workspace")
    assert kernel == "prefill_mfma_q8"
    check(out, ref)
