"""The paged-cache write fused into a PREFILL launch over an fp8 cache (library 0.6.2; csrc/prefill_lat.hip, WR && KV8): the
cache holds the bytes the separate write stores, the step's own rows are attended over as a later step reads them from the
cache, the output matches fp64 attention over the dequantised written cache. The last test is host arithmetic (no GPU)."""

import ctypes as C
import types

import pytest
import torch

import golden_io
from oracle import paged_attention_oracle as orc

gpu = pytest.mark.gpu
FP8 = [torch.float8_e4m3fn, torch.float8_e5m2]
KS, VS = 0.37, 0.61              # no powers of two: x / scale and x * (1 / scale) round differently
CASES = {                        # q_lens, kv_lens, Hq, Hk, page
    "ends_inside_a_group": ([100], [100], 32, 8, 16),                 # eight-wave form
    "straddling_group": ([130], [167], 32, 8, 16),                    # ctx 37: cache groups, the straddling one, new groups in one Q block
    "four_wave_form": ([700], [700], 32, 8, 16),                      # wgs 352 > 288, one sequence >= 640 keys; several tiles per wave
    "mixed_step": ([1, 130, 1, 64], [200, 167, 17, 64], 32, 8, 16),   # two launches, the one-token rows on the decode write
    "g1_page32": ([130], [167], 8, 8, 32),
}


def _case(seed, q_lens, kv_lens, hq, hk, page, dtype, kv_dtype, ks, vs, dev="cuda:0"):
    """Inputs on `dev`, the scales as tensors, and the caches with the slots about to be written poisoned (0x7F: NaN in both formats)."""
    inp = orc.make_paged_inputs(seed, q_lens, kv_lens, hq, hk, 128, page, dtype, kv_dtype=kv_dtype, kv_scale=ks)
    g = torch.Generator().manual_seed(seed + 100)
    inp["k_new"] = ((torch.rand(sum(q_lens), hk, 128, generator=g) * 2 - 1) * 1.2).to(dtype)
    inp["v_new"] = (torch.rand(sum(q_lens), hk, 128, generator=g) * 2 - 1).to(dtype)
    inp["slots"] = torch.tensor([int(inp["block_table"][i, p // page]) * page + p % page
                                 for i, (ql, kl) in enumerate(zip(q_lens, kv_lens)) for p in range(kl - ql, kl)])
    for c in (inp["k_cache"], inp["v_cache"]):
        c.view(torch.uint8).view(-1, hk, 128)[inp["slots"]] = 0x7F
    d_ = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return inp, d_, torch.tensor([ks], device=dev), torch.tensor([vs], device=dev)


def _separate_write(d_, slots, ks, vs):
    from mi355_attn.kernels import reshape_and_cache_flash

    kc, vc = d_["k_cache"].clone(), d_["v_cache"].clone()
    reshape_and_cache_flash(d_["k_new"], d_["v_new"], kc, vc, slots, "auto", ks, vs)
    return kc.view(torch.uint8), vc.view(torch.uint8)


def _fused(d_, slot_mapping, ks, vs):
    from mi355_attn import _lib
    from mi355_attn.kernels.unified import prefill_attention_and_cache_write

    kc, vc, out = d_["k_cache"].clone(), d_["v_cache"].clone(), torch.full_like(d_["q"], float("nan"))
    ql = (d_["cu_seqlens_q"][1:] - d_["cu_seqlens_q"][:-1]).max().item()
    assert prefill_attention_and_cache_write(d_["q"], d_["k_new"], d_["v_new"], kc, vc, out, d_["cu_seqlens_q"], ql, d_["seqused_k"],
                                             d_["seqused_k"].max().item(), d_["scale"], d_["block_table"], slot_mapping, ks, vs)
    torch.cuda.synchronize()
    assert _lib.last_kernel().startswith("prefill_mfma_lat_fp8") and not torch.isnan(out).any(), _lib.last_kernel()
    return kc.view(torch.uint8), vc.view(torch.uint8), out


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kv_dtype", FP8)
@pytest.mark.parametrize("case", list(CASES))
def test_cache_bytes_and_output(case, kv_dtype, dtype):
    """Both caches byte for byte what the separate write stores (negative slots and everything else untouched); the output
    against fp64 attention over the dequantised cache holding ALL the new rows: bf16 2e-2 / f16 1e-3, + 1e-2 for fp8."""
    inp, d_, ks, vs = _case(81, *CASES[case], dtype, kv_dtype, KS, VS)
    full = _separate_write(d_, d_["slots"], ks, vs)
    ref = orc.dense_attention_fp64(inp["q"], full[0].cpu().view(kv_dtype), full[1].cpu().view(kv_dtype), inp["cu_seqlens_q"], inp["seqused_k"],
                                   inp["block_table"], inp["scale"], k_scale=KS, v_scale=VS)
    variants = [(d_["slots"], full)]
    if case == "mixed_step":          # int64 / int32 with two padding tokens (prefill rows of two sequences), and no slot mapping
        neg = d_["slots"].clone()
        neg[[50, 140]] = -1
        holed = _separate_write(d_, neg, ks, vs)
        variants = [(neg, holed), (neg.to(torch.int32), holed), (None, full)]
    atol, rtol = golden_io.tolerance(dtype, kv_dtype)
    for slot_mapping, want in variants:
        kc, vc, out = _fused(d_, slot_mapping, ks, vs)
        assert torch.equal(kc, want[0]) and torch.equal(vc, want[1])
        err = (out.double().cpu() - ref).abs()
        print(f"{case} {kv_dtype} {dtype}: max |err| {err.max().item():.3e}")
        assert bool((err <= atol + rtol * ref.abs()).all())


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_own_rows_are_attended_over_as_the_cache_will_hold_them(dtype):
    """e5m2, ctx 0, v_scale 0.5: token 0 of every sequence sees ONE key, so its output row is v_scale * dequant(stored byte) in
    the query type, within relative 2^-7. A kernel attending over the raw 16-bit rows misses that: the raw row is off by more
    than 2^-6, twice the bound, in over half of its elements (asserted on the inputs: 68 % at least, 80 % on average. Beyond
    2^-4 it is a quarter - e5m2's rounding error is uniform up to 2^-3 relative - so that share cannot be had from U(-1, 1))."""
    inp, d_, ks, vs = _case(82, [70, 70], [70, 70], 32, 8, 16, dtype, torch.float8_e5m2, 1.0, 0.5)
    kc, vc, out = _fused(d_, d_["slots"], ks, vs)
    for s0 in (0, 70):
        stored = vc.view(torch.float8_e5m2).view(-1, 8, 128)[d_["slots"][s0]].float().cpu()              # [Hk, D]
        want = (0.5 * stored).to(dtype).float().repeat_interleave(4, dim=0)                               # per query head
        raw = inp["v_new"][s0].float().repeat_interleave(4, dim=0)
        assert ((raw - want).abs() > 2.0 ** -6 * want.abs()).float().mean(dim=-1).min() > 0.5
        assert bool(((out[s0].float().cpu() - want).abs() <= 2.0 ** -7 * want.abs()).all())


@gpu
def test_impl_forward_over_an_fp8_cache_is_one_op(monkeypatch):
    """MI355AttentionImpl.forward with kv_cache_dtype="fp8" (fused path switched on) on a 300-token prompt: the two-call path's cache bytes."""
    from mi355_attn import _lib
    from mi355_attn.backend import attn

    monkeypatch.setattr(attn, "_FUSED_PREFILL_WRITE_FP8", True)
    inp, d_, ks, vs = _case(83, [300], [300], 32, 8, 16, torch.bfloat16, torch.float8_e4m3fn, KS, VS)
    want = _separate_write(d_, d_["slots"], ks, vs)
    kv_cache = torch.stack([d_["k_cache"], d_["v_cache"]]).view(torch.uint8)
    impl = attn.MI355AttentionImpl(32, 128, inp["scale"], 8, None, None, "fp8")
    layer = types.SimpleNamespace(_k_scale=ks, _v_scale=vs, _q_scale=torch.ones((), device="cuda:0"), _q_scale_float=1.0)
    md = attn.MI355AttentionMetadata(num_actual_tokens=300, max_query_len=300, avg_query_len=300, avg_seq_len=300, query_start_loc=d_["cu_seqlens_q"],
                                     max_seq_len=300, seq_lens=d_["seqused_k"], block_table=d_["block_table"], slot_mapping=d_["slots"], use_cascade=False,
                                     common_prefix_len=0, cu_prefix_query_lens=None, prefix_kv_lens=None, suffix_kv_lens=None)
    out = torch.full((300, 32 * 128), float("nan"), dtype=torch.bfloat16, device="cuda:0")
    impl.forward(layer, d_["q"], d_["k_new"], d_["v_new"], kv_cache, md, output=out)
    torch.cuda.synchronize()
    assert _lib.last_kernel() == "prefill_mfma_lat_fp8" and not torch.isnan(out).any()
    assert torch.equal(kv_cache[0], want[0]) and torch.equal(kv_cache[1], want[1])


@pytest.mark.parametrize("kv_dtype", FP8)
def test_host_answer_for_fp8_steps(kv_dtype):
    """mi355_decode_write_fusable: 1 for an fp8 500-token prompt and for the mixed step above, 0 at 2048 keys and with a sliding
    window; where it answers 1, mi355_attn_workspace_bytes accepts the block with write_new_kv = 1 (it answers 0 both for a
    refused block and for one that needs no workspace: told apart by the error text, primed with another refusal)."""
    from mi355_attn import _lib
    from mi355_attn.kernels.unified import fill_attn_params

    h = _lib.load()

    def answer(q_lens, kv_lens, window=(-1, -1)):          # CPU tensors: host arithmetic never reads through the pointers
        inp, d_, ks, vs = _case(84, q_lens, kv_lens, 32, 8, 16, torch.bfloat16, kv_dtype, KS, VS, dev="cpu")
        args = (d_["q"], d_["k_cache"], d_["v_cache"], d_["q"], d_["cu_seqlens_q"], max(q_lens), d_["seqused_k"], max(kv_lens), 0.088, window,
                d_["block_table"], 0.0, ks, vs, None, None)
        p, keep = fill_attn_params(*args, k_new=d_["k_new"], v_new=d_["v_new"], write_new_kv=True)
        bad, _ = fill_attn_params(*args, non_causal=True, write_new_kv=True)
        h.mi355_attn_workspace_bytes(C.byref(bad))
        primed = _lib.last_error()
        h.mi355_attn_workspace_bytes(C.byref(p))
        return h.mi355_decode_write_fusable(C.byref(p)), primed.startswith("non_causal") and _lib.last_error() == primed

    assert answer([500], [500]) == (1, True) and answer(*CASES["mixed_step"][:2]) == (1, True)
    assert answer([2048], [2048]) == (0, False) and answer([500], [500], window=(127, 0)) == (0, False)
