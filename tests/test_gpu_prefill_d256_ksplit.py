"""-m gpu: the key-split form of prefill_d256_kernel / prefill_d256_fp8_kernel (csrc/prefill_d256*.hip, library 0.13.0) against
the CPU oracle. The ragged batch of tests/test_gpu_prefill_d256.py: its longest sequence has 13 key tiles, so 2 / 3 / 8 forced
splits give unequal, single-tile and empty shares, shares past a short sequence's keys and shares under the diagonal."""

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
WS_HEAD = 256 << 10        # the zero-filled head of every workspace (include/mi355_attn.h)


@functools.lru_cache(maxsize=None)
def case(dtype, kv_dtype, hq, window=0):
    """(inputs on the host, oracle output, float64 dense output, float64 dense lse) - computed once and shared."""
    sc = dict(k_scale=KS, v_scale=VS) if kv_dtype else {}
    inp = orc.make_paged_inputs(280, Q_LENS, KV_LENS, hq, 2, 256, 16, dtype, kv_dtype=kv_dtype, kv_scale=KS if kv_dtype else 1.0)
    args = (inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"], inp["scale"])
    ref = orc.unified_attention_oracle(*args, sliding_window=window, mode="2d", block_n=64, **sc)
    out64, lse64 = orc.dense_attention_fp64(*args, sliding_window=window, return_lse=True, **sc)
    return inp, ref, out64, lse64


def run(inp, q_lens, kv_lens, *, window=0, fp8=False, force=2, num_segments=0, sinks=None, skip_decodes=False):
    """One call through the C ABI on a zero-filled workspace of the size the library asks for -> (out, lse, name, workspace, bytes)."""
    from mi355_attn import _lib
    from mi355_attn.kernels.unified import fill_attn_params

    t = gpu_util.to_dev(inp)
    out = torch.full_like(t["q"], float("nan"))
    lse = torch.full(t["q"].shape[:2], float("nan"), dtype=torch.float32, device=gpu_util.DEV)
    kst, vst = (torch.tensor([KS], device=gpu_util.DEV), torch.tensor([VS], device=gpu_util.DEV)) if fp8 else (None, None)
    p, _keep = fill_attn_params(t["q"], t["k_cache"], t["v_cache"], out, t["cu_seqlens_q"], max(q_lens), t["seqused_k"], max(kv_lens), inp["scale"],
                                (window - 1, 0) if window else (-1, -1), t["block_table"], 0.0, kst, vst, None, force, num_segments=num_segments,
                                lse=lse, sinks=sinks, skip_decodes=skip_decodes)
    lib = _lib.load()
    nbytes = lib.mi355_attn_workspace_bytes(ctypes.byref(p))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=gpu_util.DEV)
    _lib.check(lib.mi355_unified_attention(ctypes.byref(p), _lib.ptr(ws), nbytes, _lib.current_stream_handle(gpu_util.DEV)), "mi355_unified_attention")
    torch.cuda.synchronize()
    return out, lse, _lib.last_kernel(), ws, nbytes


def name_of(kv_dtype, window):
    return "prefill_mfma" + ("_fp8" if kv_dtype else "") + "_d256" + ("_sw" if window else "") + "_ksplit"


def check(out, ref, dtype, kv_dtype):
    assert not torch.isnan(out).any()
    atol, rtol = golden_io.tolerance(dtype, kv_dtype)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=atol, rtol=rtol)


@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("splits", [2, 3, 8])
@pytest.mark.parametrize("dtype,kv_dtype,hq", [(BF, None, 8), (F16, None, 8), (BF, E4, 8), (F16, E5, 8), (BF, None, 6)])
def test_forced_splits_match_the_oracle(dtype, kv_dtype, hq, splits, window):
    inp, ref, _, lse64 = case(dtype, kv_dtype, hq, window)
    out, lse, name, _, _ = run(inp, Q_LENS, KV_LENS, window=window, fp8=kv_dtype is not None, num_segments=splits)
    assert name == name_of(kv_dtype, window)
    check(out, ref, dtype, kv_dtype)
    torch.testing.assert_close(lse.double().cpu(), lse64, atol=3e-2 if kv_dtype else 2e-2, rtol=1e-3)


@pytest.mark.parametrize("kv_dtype", [None, E4])
def test_stale_nan_bytes_beyond_the_sequences_are_ignored(kv_dtype):
    """Every slot no sequence uses holds NaN (16-bit) or 0x7f (NaN in e4m3fn), in both caches."""
    inp, ref, _, _ = case(BF, kv_dtype, 8)
    inp = dict(inp, k_cache=inp["k_cache"].clone(), v_cache=inp["v_cache"].clone())
    used = torch.zeros(inp["k_cache"].shape[:2], dtype=torch.bool)
    for i, n in enumerate(KV_LENS):
        for j in range(n):
            used[inp["block_table"][i, j // 16], j % 16] = True
    for key in ("k_cache", "v_cache"):
        if kv_dtype:
            inp[key].view(torch.uint8)[~used] = 0x7F
        else:
            inp[key][~used] = float("nan")
    out, _, name, _, _ = run(inp, Q_LENS, KV_LENS, fp8=kv_dtype is not None, num_segments=3)
    assert name == name_of(kv_dtype, 0)
    check(out, ref, BF, kv_dtype)


@pytest.mark.parametrize("window", [0, 100])
def test_sinks_and_lse(window):
    """The partials are sink-free and the merge adds exp(sinks[h]) to the denominator once: in float64, from the sink-free
    dense result, lse = log(exp(lse0) + exp(sink)) and out = out0 * exp(lse0 - lse)."""
    inp, _, out0, lse0 = case(BF, None, 8, window)
    sinks = torch.linspace(-2.0, 2.0, 8)[torch.randperm(8, generator=torch.Generator().manual_seed(281))]
    ref_lse = torch.logaddexp(lse0, sinks.double()[None, :])
    ref = out0 * torch.exp(lse0 - ref_lse)[..., None]
    out, lse, name, _, _ = run(inp, Q_LENS, KV_LENS, window=window, num_segments=3, sinks=sinks)
    assert name == name_of(None, window)
    check(out, ref, BF, None)
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double().cpu(), ref_lse, atol=2e-2, rtol=0)


@pytest.mark.parametrize("q_lens,ctx_lens", [([300], [3800]), ([1, 200, 1], [777, 3900, 40])])
def test_auto_dispatch_and_workspace(q_lens, ctx_lens):
    """The default plan (AUTO, no num_segments): a chunk over ~4000 context keys, alone and as the prefill half of a mixed step.
    The prefill launch's workspace is the documented layout for the plan's split count - the 256 KiB head, `splits` partial
    outputs in the query type rounded up to 256 bytes, `splits` f32 partial lse's; a mixed step asks for the larger of that and
    its decode launch's - and the head is zero again afterwards."""
    kv_lens = [a + b for a, b in zip(q_lens, ctx_lens)]
    inp = orc.make_paged_inputs(282, q_lens, kv_lens, 8, 2, 256, 16, BF)
    args = (inp["q"], inp["k_cache"], inp["v_cache"], inp["cu_seqlens_q"], inp["seqused_k"], inp["block_table"], inp["scale"])
    ref = orc.unified_attention_oracle(*args, mode="2d", block_n=64)
    if len(q_lens) > 1:      # query_len == 1 rows run on the split-KV decode kernel: the 3D restatement is their oracle
        ref3 = orc.unified_attention_oracle(*args, mode="3d")
        for row in (0, 201):
            ref[row] = ref3[row]
    out, _, name, ws, nbytes = run(inp, q_lens, kv_lens, force=None)
    prefill, _, decode = name.partition("+")
    assert prefill == "prefill_mfma_d256_ksplit" and decode.startswith("decode_") == (len(q_lens) > 1), name
    # plan_key_splits(): fewer than 512 workgroups over >= 32 tiles -> min(ceil(512 / workgroups), tiles / 8, 8) splits, evened out
    tokens, tiles = sum(q_lens), (max(kv_lens) + 63) // 64
    wgs = (tokens // 32 + len(q_lens)) * 2
    splits = min(-(-512 // wgs), tiles // 8, 8)
    splits = -(-tiles // -(-tiles // splits))
    rows = tokens * 8
    prefill_bytes = run(inp, q_lens, kv_lens, force=None, skip_decodes=True)[4] if decode else nbytes
    assert nbytes >= prefill_bytes == WS_HEAD + ((splits * rows * 256 * 2 + 255) & ~255) + splits * rows * 4
    assert not ws[:WS_HEAD].any()
    check(out, ref, BF, None)
