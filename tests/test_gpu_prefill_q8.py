"""-m gpu: prefill_q8_kernel (csrc/prefill_q8.hip) - e4m3 queries over an fp8 cache at head size 128, bf16 output - against
float64 dense attention on the dequantised inputs. Ragged batch: one-row and one-key sequences, 129 / 257 keys (one past a tile).
Tolerance: rtol the project's bf16 2e-2; atol twice the largest error of a CPU emulation (128-key tiles, running maximum, fp32
accumulation, bf16 output) on exactly these inputs. P rounded to e4m3 ONCE (the reference's P.to(V.dtype)) measured 4.3e-2, peaked
1.0e-1; with P scaled by 2^8 and the row sum from the rounded P 4.3e-2 / 9.8e-2 - an atol of 0.2 where the peaked case may take
5e-2 at most. The kernel therefore feeds P as two e4m3 terms (rounded weight + rounded residual): emulated 4.3e-3 / 1.7e-2 (peaked)
-> atol 9e-3 / 3.4e-2."""

import ctypes
import functools

import pytest
import torch

import gpu_util
from oracle import paged_attention_oracle as orc

pytestmark = pytest.mark.gpu

BF, E4, E5 = torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2
Q_LENS, KV_LENS = [1, 5, 129, 1, 64, 200], [9, 5, 129, 300, 257, 777]
KS, VS = 0.0237, 0.041
ATOL, ATOL_PEAKED, RTOL = 9e-3, 3.4e-2, 2e-2

@functools.lru_cache(maxsize=None)
def case(kv_dtype, hq, hk, page, window=0, max_value=1.0):
    """(inputs on the host with q in e4m3, float64 output, float64 lse) - computed once per configuration and shared."""
    inp = orc.make_paged_inputs(310, Q_LENS, KV_LENS, hq, hk, 128, page, BF, kv_dtype=kv_dtype, kv_scale=KS, max_value=max_value)
    inp["q"] = inp["q"].to(E4)
    ref, lse = orc.dense_attention_fp64(inp["q"].float(), inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"],
                                        inp["scale"], sliding_window=window, k_scale=KS, v_scale=VS, return_lse=True)
    return inp, ref, lse


def run(inp, window=0, force=2):
    t = gpu_util.to_dev(inp)
    out = torch.full(t["q"].shape, float("nan"), dtype=BF, device=gpu_util.DEV)
    return gpu_util.run_unified(t, inp["scale"], window=window, kv_scale=KS, v_scale=VS, force=force, out=out)


def run_params(inp, window=0, **kw):
    """The same through fill_attn_params (lse, sinks, skip_decodes): (out, kernel, workspace bytes)."""
    from mi355_attn import _lib
    from mi355_attn.kernels import unified

    t = gpu_util.to_dev(inp)
    out = torch.full(t["q"].shape, float("nan"), dtype=BF, device=gpu_util.DEV)
    kst, vst = torch.tensor([KS], device=gpu_util.DEV), torch.tensor([VS], device=gpu_util.DEV)
    p, _keep = unified.fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], max(Q_LENS), t["seqused_k"], max(KV_LENS), inp["scale"],
                                        (window - 1, 0) if window else None, t["block_table"], 0.0, kst, vst, None, 2, **kw)
    nbytes = _lib.load().mi355_attn_workspace_bytes(ctypes.byref(p))
    unified.launch(p, gpu_util.DEV)
    torch.cuda.synchronize()
    return out, _lib.last_kernel(), nbytes


def check(out, ref, atol=ATOL):
    assert not torch.isnan(out).any()
    print(f"max|err| {(out.double().cpu() - ref).abs().max():.3e} (atol {atol})")
    torch.testing.assert_close(out.double().cpu(), ref, atol=atol, rtol=RTOL)


@pytest.mark.parametrize("kv_dtype,hq,hk,page,max_value", [(kv, *c, 1.0) for kv in (E4, E5) for c in ((8, 2, 32), (6, 2, 32), (16, 1, 128))] + [(E4, 8, 2, 32, 3.0)])
def test_plain_matches_float64(kv_dtype, hq, hk, page, max_value):
    """max_value 3.0, the peaked case: outputs of unit size carried by a few keys each."""
    inp, ref, _ = case(kv_dtype, hq, hk, page, max_value=max_value)
    out, kernel = run(inp)
    assert kernel == "prefill_mfma_q8"
    check(out, ref, ATOL if max_value == 1.0 else ATOL_PEAKED)


@pytest.mark.parametrize("window", [8, 128, 200, 300])
def test_sliding_window_matches_float64(window):
    """A window inside one tile, on the tile edge, across tiles, longer than most sequences."""
    inp, ref, _ = case(E4, 8, 2, 32, window)
    out, kernel = run(inp, window)
    assert kernel == "prefill_mfma_q8_sw"
    check(out, ref)


def test_stale_nan_bytes_beyond_the_sequences_are_ignored():
    """0x7f is NaN in e4m3fn: every slot no sequence uses holds it, in both caches."""
    inp, ref, _ = case(E4, 8, 2, 32)
    inp = dict(inp, k_cache=inp["k_cache"].clone(), v_cache=inp["v_cache"].clone())
    used = torch.zeros(inp["k_cache"].shape[:2], dtype=torch.bool)
    for i, n in enumerate(KV_LENS):
        for j in range(n):
            used[inp["block_table"][i, j // 32], j % 32] = True
    for name in ("k_cache", "v_cache"):
        inp[name].view(torch.uint8)[~used] = 0x7F
    out, kernel = run(inp)
    assert kernel == "prefill_mfma_q8"
    check(out, ref)


@pytest.mark.parametrize("window", [0, 100])
def test_sinks_and_lse(window):
    """From the sink-free float64 result: lse = log(exp(lse0) + exp(sink)), out = out0 * exp(lse0 - lse)."""
    inp, out0, lse0 = case(E4, 8, 2, 32, window)
    sinks = torch.linspace(-2.0, 2.0, 8)[torch.randperm(8, generator=torch.Generator().manual_seed(311))]
    ref_lse = torch.logaddexp(lse0, sinks.double()[None, :])
    lse = torch.full(inp["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    out, kernel, _ = run_params(inp, window, lse=lse, sinks=sinks.to(gpu_util.DEV))
    assert kernel == ("prefill_mfma_q8_sw" if window else "prefill_mfma_q8")
    check(out, out0 * torch.exp(lse0 - ref_lse)[..., None])
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double().cpu(), ref_lse, atol=2e-2, rtol=0)


def test_skip_decodes_leaves_the_one_token_rows():
    """Without skip_decodes the same launch writes the one-token rows too (no second kernel behind a '+'), under AUTO as well."""
    inp, ref, _ = case(E4, 8, 2, 32)
    out, kernel = run(inp, force=None)
    assert kernel == "prefill_mfma_q8"
    check(out, ref)
    out, kernel, nbytes = run_params(inp, skip_decodes=True)
    assert kernel == "prefill_mfma_q8" and nbytes == 0
    keep = torch.ones(sum(Q_LENS), dtype=torch.bool)
    keep[[0, 135]] = False                                  # the tokens of the two one-token sequences
    assert torch.isnan(out.cpu()[~keep]).all()
    check(out.cpu()[keep], ref[keep])
