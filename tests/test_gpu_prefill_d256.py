"""-m gpu: prefill_d256_kernel (csrc/prefill_d256.hip) - causal prefill at head size 256, plain or with a sliding window -
against the CPU oracle. The ragged batch has one-row and one-key sequences, a Q block that straddles two sequences, a
partial last tile, tiles on the diagonal and, at Hq 6 / Hk 2, a group size that is no power of two."""

import ctypes
import functools

import pytest
import torch

import golden_io
import gpu_util
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
Q_LENS, KV_LENS = [1, 5, 129, 1, 64, 200], [9, 5, 129, 300, 257, 777]


@functools.lru_cache(maxsize=None)
def case(dtype, hq, hk, page=16, window=0):
    """(inputs on the host, oracle output) - computed once per configuration and shared."""
    inp = orc.make_paged_inputs(256, Q_LENS, KV_LENS, hq, hk, 256, page, dtype)
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                       inp["scale"], sliding_window=window, mode="2d", block_n=64)
    return inp, ref


def check(out, ref, dtype):
    assert not torch.isnan(out).any()
    atol, rtol = golden_io.tolerance(dtype)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("hq,hk,page", [(8, 2, 16), (4, 4, 16), (6, 2, 16), (16, 1, 16), (8, 2, 128)])
@pytest.mark.parametrize("dtype", [BF, F16])
def test_plain_matches_the_oracle(dtype, hq, hk, page):
    inp, ref = case(dtype, hq, hk, page)
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], force=2)
    assert kernel == "prefill_mfma_d256"
    check(out, ref, dtype)


@pytest.mark.parametrize("window", [8, 64, 100, 300])
@pytest.mark.parametrize("dtype", [BF, F16])
def test_sliding_window_matches_the_oracle(dtype, window):
    """A window inside one tile, on a tile edge, over several tiles, longer than most sequences."""
    inp, ref = case(dtype, 8, 2, 16, window)
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], window=window, force=2)
    assert kernel == "prefill_mfma_d256_sw"
    check(out, ref, dtype)


@pytest.mark.parametrize("window", [0, 100])
def test_sinks_and_lse(window):
    """exp(sinks[h]) joins the denominator (include/mi355_attn.h): in float64, from the sink-free dense result,
    lse = log(exp(lse0) + exp(sink)) and out = out0 * exp(lse0 - lse)."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified_attention_with_sinks

    inp, _ = case(BF, 8, 2, 16, window)
    out0, lse0 = orc.dense_attention_fp64(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                          inp["scale"], sliding_window=window, return_lse=True)
    sinks = torch.linspace(-2.0, 2.0, 8)[torch.randperm(8, generator=torch.Generator().manual_seed(257))]
    ref_lse = torch.logaddexp(lse0, sinks.double()[None, :])
    ref = out0 * torch.exp(lse0 - ref_lse)[..., None]
    t = gpu_util.to_dev(inp)
    out = torch.full_like(t["q"], float("nan"))
    lse = torch.full(t["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    unified_attention_with_sinks(
        q=t["q"], k=t["k_cache"], v=t["v_cache"], out=out, cu_seqlens_q=t["cu_seqlens_q"], max_seqlen_q=max(Q_LENS), seqused_k=t["seqused_k"],
        max_seqlen_k=max(KV_LENS), avg_seqlen_q=0, avg_seqlen_k=0, softmax_scale=inp["scale"], causal=True,
        window_size=(window - 1, 0) if window else (-1, -1), block_table=t["block_table"], softcap=0, q_descale=None, k_descale=None,
        v_descale=None, force_selection=2, softmax_lse=lse, sinks=sinks.to(gpu_util.DEV))
    torch.cuda.synchronize()
    assert _lib.last_kernel() == ("prefill_mfma_d256_sw" if window else "prefill_mfma_d256")
    check(out, ref, BF)
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double().cpu(), ref_lse, atol=2e-2, rtol=0)      # tests/test_gpu_sinks.py


def test_f16_score_that_rises_late():
    """200 query tokens over 777 keys: key 640 - the first of the eleventh tile of thirteen, the latest keys of the rows that see it -
    scores 30 nats (43 in base 2) above everything before it in every row of KV head 0. The running maximum absorbs it."""
    inp = orc.make_paged_inputs(258, [200], [777], 8, 2, 256, 16, F16)
    direction = torch.nn.functional.normalize(torch.randn(256, generator=torch.Generator().manual_seed(259)), dim=0)
    inp["k_cache"][int(inp["block_table"][0, 640 // 16]), 640 % 16, 0] = (direction * 8.0).to(F16)
    inp["q"][:, :4] = (inp["q"][:, :4].float() * 0.25 + direction * (30.0 / inp["scale"] / 8.0)).to(F16)
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                       inp["scale"], mode="2d", block_n=64)
    out, kernel = gpu_util.run_unified(gpu_util.to_dev(inp), inp["scale"], force=2)
    assert kernel == "prefill_mfma_d256"
    assert torch.isfinite(out).all()
    check(out, ref, F16)


def test_auto_dispatch_and_skip_decodes():
    """The smallest shape the AUTO rule sends here: 512 keys (kD256MinKeys, prefill_mfma.hip), 8 key tiles - no key-split plan,
    no workspace. With skip_decodes = 1 the call is one launch of this kernel and leaves the one-token row alone; without it
    the step is a mixed one, whose prefill rows run here and whose one-token row runs on the decode kernel behind a '+'."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified

    q_lens, kv_lens = [1, 512], [40, 512]
    inp = orc.make_paged_inputs(260, q_lens, kv_lens, 8, 2, 256, 16, BF)
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                       inp["scale"], mode="2d", block_n=64)
    t = gpu_util.to_dev(inp)
    out, kernel = gpu_util.run_unified(t, inp["scale"])
    assert kernel.split("+")[0] == "prefill_mfma_d256", kernel
    check(out, ref, BF)

    out = torch.full_like(t["q"], float("nan"))
    p, _keep = unified.fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], max(q_lens), t["seqused_k"], max(kv_lens), inp["scale"],
                                        None, t["block_table"], 0.0, None, None, None, None, skip_decodes=True)
    assert _lib.load().mi355_attn_workspace_bytes(ctypes.byref(p)) == 0
    unified.launch(p, gpu_util.DEV)
    torch.cuda.synchronize()
    assert _lib.last_kernel() == "prefill_mfma_d256"
    assert torch.isnan(out[0]).all()
    check(out[1:], ref[1:], BF)
