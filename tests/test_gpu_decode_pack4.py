"""-m gpu: multi-token decode rows of up to 64 / G tokens on four column groups (`decode_rows_hint`, library 0.8.0) against
the CPU oracle: a uniform speculative step in one launch, a mixed step's decode launch, and the fallbacks that keep their
former kernels."""

import pytest
import torch

import golden_io
import gpu_util
from mi355_attn import _lib
from mi355_attn.kernels import unified_attention_with_sinks
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu


def _attend(d, inp, q_lens, kv_lens, *, hint=0, window=0, sinks=None, force=None):
    """One call on NaN-filled outputs -> (out, lse, kernel)."""
    out = torch.full_like(d["q"], float("nan"))
    lse = torch.full(d["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    ks = None if inp["kv_scale"] is None else torch.tensor([inp["kv_scale"]], dtype=torch.float32, device=gpu_util.DEV)
    unified_attention_with_sinks(
        q=d["q"], k=d["k_cache"], v=d["v_cache"], out=out, cu_seqlens_q=d["cu_seqlens_q"], max_seqlen_q=max(q_lens), seqused_k=d["seqused_k"],
        max_seqlen_k=max(kv_lens), avg_seqlen_q=1, avg_seqlen_k=1, softmax_scale=inp["scale"], causal=True,
        window_size=(window - 1, 0) if window else (-1, -1), block_table=d["block_table"], softcap=0, q_descale=None, k_descale=ks, v_descale=ks,
        force_selection=force, softmax_lse=lse, decode_rows_hint=hint, sinks=sinks)
    torch.cuda.synchronize()
    return out, lse, _lib.last_kernel()


def _check(q_lens, kv_lens, hq, hk, d_head, dtype, *, hint, kv_dtype=None, kv_scale=None, window=0, with_sinks=False, seed=81):
    inp = orc.make_paged_inputs(seed, q_lens, kv_lens, hq, hk, d_head, 16, dtype, kv_dtype=kv_dtype, kv_scale=kv_scale or 1.0)
    inp["kv_scale"] = kv_scale
    ref = orc.unified_attention_oracle(inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"], inp["scale"],
                                       sliding_window=window, k_scale=kv_scale or 1.0, v_scale=kv_scale or 1.0, mode="2d", block_n=64).float()
    d = gpu_util.to_dev(inp)
    sinks = torch.linspace(-8.0, 8.0, hq, device=gpu_util.DEV) if with_sinks else None     # a per-head ramp
    out, lse, kernel = _attend(d, inp, q_lens, kv_lens, hint=hint, window=window, sinks=sinks)
    _, lse_ref, _ = _attend(d, inp, q_lens, kv_lens, window=window, sinks=sinks, force=9)
    if with_sinks:      # the oracle has no sinks: a sink scales a row by L / (L + exp(sink)), L = exp(the row's sink-free lse)
        _, lse0, _ = _attend(d, inp, q_lens, kv_lens, window=window, force=9)
        ref = ref * torch.sigmoid(lse0.cpu() - sinks.cpu())[..., None]
    atol, rtol = golden_io.tolerance(dtype, kv_dtype)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), kernel
    torch.testing.assert_close(out.float().cpu(), ref, atol=atol, rtol=rtol, msg=lambda m: f"[{kernel}] {m}")
    torch.testing.assert_close(lse, lse_ref, atol=2e-2 if kv_dtype is None else 3e-2, rtol=1e-3, msg=lambda m: f"[{kernel}] lse {m}")
    return kernel


@pytest.mark.parametrize("hq,hk,d_head,dtype,kv_dtype,hint,with_sinks", [
    (64, 8, 128, torch.bfloat16, None, 8, False),
    (64, 8, 64, torch.bfloat16, None, 8, True),
    (32, 8, 128, torch.float16, None, 16, False),
    (32, 2, 128, torch.bfloat16, None, 4, False),                      # G = 16
    (12, 2, 128, torch.bfloat16, None, 8, False),                      # G = 6: 8 tokens per unit, a token's columns straddle the 16-column groups
    (64, 8, 128, torch.float16, torch.float8_e4m3fn, 8, False),
])
def test_uniform_speculative_step_is_one_launch_on_four_column_groups(hq, hk, d_head, dtype, kv_dtype, hint, with_sinks):
    """Rows of up to `hint` tokens: no context at all (the causal staircase alone), a short context, one token, many splits
    (the merge launch), exactly one tile (the last token's diagonal on the tile edge), a ragged row."""
    q_lens = [max(1, q) for q in (hint, hint - 3, 1, hint - 1, hint, 2)]
    kv_lens = [q_lens[0], 5 + q_lens[1], 17, 2048 + q_lens[3], 64, 513 + q_lens[5]]
    kernel = _check(q_lens, kv_lens, hq, hk, d_head, dtype, hint=hint, kv_dtype=kv_dtype, kv_scale=0.5 if kv_dtype else None, with_sinks=with_sinks)
    assert "pack4" in kernel and "+" not in kernel and ("fp8" in kernel) == (kv_dtype is not None), kernel


def test_mixed_step_sends_rows_of_up_to_the_hint_to_the_decode_launch():
    """Prefill chunks (300 and 64 tokens) with verification rows of 1 .. 8 tokens: every row exactly once (NaN-filled output)."""
    kernel = _check([300, 8, 1, 5, 64, 7, 1], [900, 640, 17, 2048, 64, 333, 513], 64, 8, 128, torch.bfloat16, hint=8, seed=82)
    assert "+decode" in kernel and "pack4" in kernel, kernel


@pytest.mark.parametrize("d_head,hint,window", [(128, 8, 100), (256, 8, 0), (128, 0, 0)])
def test_what_four_column_groups_do_not_serve_keeps_its_kernel(d_head, hint, window):
    kernel = _check([8, 5, 1, 7, 8, 2], [8, 10, 17, 2055, 64, 515], 64, 8, d_head, torch.bfloat16, hint=hint, window=window, seed=83)
    assert "pack4" not in kernel, kernel
