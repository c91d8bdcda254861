"""CPU-only: the host side of fp8 queries (library 0.11.0) through the C ABI with dummy aligned addresses (nothing is read)."""

import ctypes as C

import pytest
import torch

from test_cpu_sinks import _params as _bf16_params, addr, lib  # noqa: F401  (the fixtures and the Hq 32 / Hk 8 / D 128 block)


def _params(lib, addr):
    """e4m3 queries over an e4m3 flash-layout cache of 32-slot pages: 4 prompts of 512 tokens and 4 decode rows."""
    p = _bf16_params(lib, addr, 4 * 512 + 4, 8, 512, 4096)
    p.q_dtype = p.kv_dtype = lib.FP8_E4M3
    p.page_size, p.k_stride_page, p.v_stride_page = 32, 32768, 32768
    return p


def _set(**kw):
    return lambda p, addr: [setattr(p, k, addr if v == "addr" else v) for k, v in kw.items()]


@pytest.mark.parametrize("change,cause", [
    (_set(), None), (_set(sliding_window=1024), None),
    (_set(q_dtype=4), "e5m2 queries"), (_set(head_size=64, k_x=64), "head size 128"), (_set(softcap=30.0), "soft-cap"),
    (_set(alibi_slopes="addr"), "ALiBi"), (_set(non_causal=1), "non_causal"), (_set(k_new="addr", v_new="addr"), "k_new"),
    (_set(write_new_kv=1), "write_new_kv"), (_set(kernel_select=3), "MI355_SELECT_3D"), (_set(kernel_select=9), "MI355_SELECT_GENERIC"),
    (_set(k_x=8, k_stride_dx=256), "legacy layout"), (_set(num_segments=4), "num_segments"), (_set(page_size=16), "page size"),
    (_set(k_stride_slot=1032), "multiple of 16")])
def test_what_is_served_and_refused_with_fp8_queries(lib, addr, change, cause):
    """Served (cause None) or refused by name before any HIP call; no workspace and no fused cache write either way."""
    h, p = lib.load(), _params(lib, addr)
    change(p, addr)
    assert h.mi355_attn_workspace_bytes(C.byref(p)) == 0 and h.mi355_decode_write_fusable(C.byref(p)) == 0
    if cause:
        assert h.mi355_unified_attention(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED
        assert cause in lib.last_error(), lib.last_error()


def test_the_legacy_entry_points_refuse_fp8_queries(lib, addr):
    h, p = lib.load(), _params(lib, addr)
    p.num_tokens, p.num_seqs, p.max_seqlen_q = 8, 8, 1
    assert h.mi355_paged_attention_v0(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED and "fp8 queries" in lib.last_error()
    p.k_new = p.v_new = addr
    assert h.mi355_context_attention_fwd_v0(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED and "fp8 queries" in lib.last_error()


def test_fill_attn_params_wants_a_bf16_out_with_fp8_queries(lib):
    from mi355_attn.kernels import unified

    q, kc = torch.zeros(4, 8, 128).to(torch.float8_e4m3fn), torch.zeros(2, 32, 2, 128).to(torch.float8_e4m3fn)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    args = (i32(0, 4), 4, i32(4), 4, 0.088, (-1, -1), i32(0).view(1, 1), 0.0, None, None, None, None)
    with pytest.raises(ValueError, match="bfloat16"):
        unified.fill_attn_params(q, kc, kc, torch.zeros(4, 8, 128, dtype=torch.float16), *args)
    p, _ = unified.fill_attn_params(q, kc, kc, torch.zeros(4, 8, 128, dtype=torch.bfloat16), *args)
    assert p.q_dtype == lib.FP8_E4M3 and p.out_stride_token == 8 * 128
