"""-m gpu: prefill_d256_fp8_kernel (csrc/prefill_d256_fp8.hip) - causal prefill at head size 256 over an fp8 cache, plain or with
a sliding window - against the CPU oracle. The ragged batch has one-row and one-key sequences, a Q block that straddles two
sequences, a partial last tile and tiles on the diagonal; the k / v scales differ and are no powers of two."""

import ctypes
import functools

import pytest
import torch

import golden_io
import gpu_util
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu

BF, F16, E4, E5 = torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2
Q_LENS, KV_LENS = [1, 5, 129, 1, 64, 200], [9, 5, 129, 300, 257, 777]
KS, VS = 0.0237, 0.041
AUTO_MIN_KEYS = 512        # kD256Fp8MinKeys, csrc/prefill_mfma.hip


@functools.lru_cache(maxsize=None)
def case(dtype, kv_dtype, hq, hk, page=16, window=0):
    """(inputs on the host, oracle output) - computed once per configuration and shared."""
    inp = orc.make_paged_inputs(270, Q_LENS, KV_LENS, hq, hk, 256, page, dtype, kv_dtype=kv_dtype, kv_scale=KS)
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                       inp["scale"], sliding_window=window, k_scale=KS, v_scale=VS, mode="2d", block_n=64)
    return inp, ref


def check(out, ref, dtype, kv_dtype):
    assert not torch.isnan(out).any()
    atol, rtol = golden_io.tolerance(dtype, kv_dtype)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("hq,hk,page", [(8, 2, 16), (6, 2, 16), (16, 1, 16), (8, 2, 128)])
@pytest.mark.parametrize("kv_dtype", [E4, E5])
@pytest.mark.parametrize("dtype", [BF, F16])
def test_plain_matches_the_oracle(dtype, kv_dtype, hq, hk, page):
    inp, ref = case(dtype, kv_dtype, hq, hk, page)
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], kv_scale=KS, v_scale=VS, force=2)
    assert kernel == "prefill_mfma_fp8_d256"
    check(out, ref, dtype, kv_dtype)


@pytest.mark.parametrize("window", [8, 64, 100, 300])
@pytest.mark.parametrize("dtype,kv_dtype", [(BF, E4), (F16, E5)])
def test_sliding_window_matches_the_oracle(dtype, kv_dtype, window):
    """A window inside one tile, on a tile edge, over several tiles, longer than most sequences."""
    inp, ref = case(dtype, kv_dtype, 8, 2, 16, window)
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], window=window, kv_scale=KS, v_scale=VS, force=2)
    assert kernel == "prefill_mfma_fp8_d256_sw"
    check(out, ref, dtype, kv_dtype)


def test_stale_nan_bytes_beyond_the_sequences_are_ignored():
    """0x7f is NaN in e4m3fn: every slot no sequence uses holds it, in both caches."""
    inp, ref = case(BF, E4, 8, 2)
    inp = dict(inp, k_cache=inp["k_cache"].clone(), v_cache=inp["v_cache"].clone())
    used = torch.zeros(inp["k_cache"].shape[:2], dtype=torch.bool)
    for i, n in enumerate(KV_LENS):
        for j in range(n):
            used[inp["block_table"][i, j // 16], j % 16] = True
    for name in ("k_cache", "v_cache"):
        inp[name].view(torch.uint8)[~used] = 0x7F
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], kv_scale=KS, v_scale=VS, force=2)
    assert kernel == "prefill_mfma_fp8_d256"
    check(out, ref, BF, E4)


@pytest.mark.parametrize("window", [0, 100])
def test_sinks_and_lse(window):
    """exp(sinks[h]) joins the denominator (include/mi355_attn.h): in float64 on the dequantised cache, from the sink-free
    dense result, lse = log(exp(lse0) + exp(sink)) and out = out0 * exp(lse0 - lse)."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified_attention_with_sinks

    inp, _ = case(BF, E4, 8, 2, 16, window)
    out0, lse0 = orc.dense_attention_fp64(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                          inp["scale"], sliding_window=window, k_scale=KS, v_scale=VS, return_lse=True)
    sinks = torch.linspace(-2.0, 2.0, 8)[torch.randperm(8, generator=torch.Generator().manual_seed(271))]
    ref_lse = torch.logaddexp(lse0, sinks.double()[None, :])
    ref = out0 * torch.exp(lse0 - ref_lse)[..., None]
    t = gpu_util.to_dev(inp)
    out = torch.full_like(t["q"], float("nan"))
    lse = torch.full(t["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    unified_attention_with_sinks(
        q=t["q"], k=t["k_cache"], v=t["v_cache"], out=out, cu_seqlens_q=t["cu_seqlens_q"], max_seqlen_q=max(Q_LENS), seqused_k=t["seqused_k"],
        max_seqlen_k=max(KV_LENS), avg_seqlen_q=0, avg_seqlen_k=0, softmax_scale=inp["scale"], causal=True,
        window_size=(window - 1, 0) if window else (-1, -1), block_table=t["block_table"], softcap=0, q_descale=None,
        k_descale=torch.tensor([KS], device=gpu_util.DEV), v_descale=torch.tensor([VS], device=gpu_util.DEV),
        force_selection=2, softmax_lse=lse, sinks=sinks.to(gpu_util.DEV))
    torch.cuda.synchronize()
    assert _lib.last_kernel() == ("prefill_mfma_fp8_d256_sw" if window else "prefill_mfma_fp8_d256")
    check(out, ref, BF, E4)
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double().cpu(), ref_lse, atol=2e-2, rtol=0)      # tests/test_gpu_sinks.py


def test_auto_dispatch_and_skip_decodes():
    """The smallest shape the AUTO rule sends here: AUTO_MIN_KEYS keys - no key-split plan, no workspace. With skip_decodes = 1
    the call is one launch of this kernel and leaves the one-token row alone; without it the step is a mixed one, whose prefill
    rows run here and whose one-token row runs on the fp8 decode kernel behind a '+'."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified

    q_lens, kv_lens = [1, AUTO_MIN_KEYS], [40, AUTO_MIN_KEYS]
    inp = orc.make_paged_inputs(272, q_lens, kv_lens, 8, 2, 256, 16, BF, kv_dtype=E4, kv_scale=KS)
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                       inp["scale"], k_scale=KS, v_scale=VS, mode="2d", block_n=64)
    t = gpu_util.to_dev(inp)
    out, kernel = gpu_util.run_unified(t, inp["scale"], kv_scale=KS, v_scale=VS)
    prefill, decode = kernel.split("+")
    assert prefill == "prefill_mfma_fp8_d256" and decode.startswith("decode_") and decode.endswith("_fp8"), kernel
    check(out, ref, BF, E4)

    out = torch.full_like(t["q"], float("nan"))
    kst, vst = torch.tensor([KS], device=gpu_util.DEV), torch.tensor([VS], device=gpu_util.DEV)
    p, _keep = unified.fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], max(q_lens), t["seqused_k"], max(kv_lens), inp["scale"],
                                        None, t["block_table"], 0.0, kst, vst, None, None, skip_decodes=True)
    assert _lib.load().mi355_attn_workspace_bytes(ctypes.byref(p)) == 0
    unified.launch(p, gpu_util.DEV)
    torch.cuda.synchronize()
    assert _lib.last_kernel() == "prefill_mfma_fp8_d256"
    assert torch.isnan(out[0]).all()
    check(out[1:], ref[1:], BF, E4)
