"""CPU-only: the host side of attention sinks (library 0.7.0) through the loaded library - where the field sits, what is
refused with it, and that the plan of a call (its workspace) does not depend on it."""

import ctypes as C
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mi355_attn import _lib

    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib


def _params(lib, addr, tokens, seqs, max_q, max_k):
    """Hq 32 / Hk 8 / D 128 bf16 over a flash-layout cache; every pointer the same non-NULL aligned address (nothing is read)."""
    p = lib.AttnParams()
    for f in ("q", "out", "k_cache", "v_cache", "block_table", "cu_seqlens_q", "seqused_k"):
        setattr(p, f, addr)
    p.q_dtype = p.kv_dtype = lib.BF16
    p.num_q_heads, p.num_kv_heads, p.head_size, p.page_size = 32, 8, 128, 16
    p.q_stride_token, p.q_stride_head, p.out_stride_token, p.out_stride_head = 4096, 128, 4096, 128
    p.k_stride_page, p.k_stride_slot, p.k_stride_head, p.k_stride_d, p.k_x = 16384, 1024, 128, 1, 128
    p.v_stride_page, p.v_stride_slot, p.v_stride_head, p.v_stride_d = 16384, 1024, 128, 1
    p.block_table_stride = 2048
    p.scale = 0.088
    p.num_tokens, p.num_seqs, p.max_seqlen_q, p.max_seqlen_k = tokens, seqs, max_q, max_k
    return p


@pytest.fixture()
def addr():
    buf = np.zeros(64, dtype=np.uint8)
    yield (buf.ctypes.data + 15) & ~15
    del buf


def test_sinks_is_the_last_field_and_the_version_says_so(lib):
    name, _ = lib.AttnParams._fields_[-1]
    assert name == "sinks"
    assert lib.AttnParams.sinks.offset + C.sizeof(C.c_void_p) == C.sizeof(lib.AttnParams)
    assert lib.load().mi355_attn_version() >= 700


def test_what_is_refused_with_sinks(lib, addr):
    h = lib.load()
    p = _params(lib, addr, 64, 64, 1, 8192)
    p.k_new = p.v_new = addr
    p.new_stride_token, p.new_stride_head = 1024, 128
    assert h.mi355_decode_write_fusable(C.byref(p)) == 1            # a decode step whose cache write is fused ...
    p.sinks = addr
    assert h.mi355_decode_write_fusable(C.byref(p)) == 0            # ... but not with sinks
    p.write_new_kv = 1
    assert h.mi355_unified_attention(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED
    assert "sinks" in lib.last_error()
    p.write_new_kv = 0
    assert h.mi355_context_attention_fwd_v0(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED
    assert "sinks" in lib.last_error()
    p.k_new = p.v_new = None
    assert h.mi355_paged_attention_v0(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED
    assert "sinks" in lib.last_error()
    p.non_causal = 1
    assert h.mi355_unified_attention(C.byref(p), None, 0, None) == lib.MI355_ERR_UNSUPPORTED
    assert "sinks" in lib.last_error()


@pytest.mark.parametrize("block,needs_scratch", [
    ("decode", True), ("short_prefill", False), ("long_prefill", False), ("key_split", True), ("mixed", True), ("generic_f32", False)])
def test_workspace_bytes_does_not_depend_on_sinks(lib, addr, block, needs_scratch):
    h = lib.load()
    p = {"decode": lambda: _params(lib, addr, 64, 64, 1, 8192),
         "short_prefill": lambda: _params(lib, addr, 512, 1, 512, 512),
         "long_prefill": lambda: _params(lib, addr, 4096, 1, 4096, 4096),
         "key_split": lambda: _params(lib, addr, 512, 1, 512, 8192),
         "mixed": lambda: _params(lib, addr, 4 * 512 + 4, 8, 512, 4096),
         "generic_f32": lambda: _params(lib, addr, 64, 64, 1, 8192)}[block]()
    if block == "generic_f32":
        p.q_dtype = p.kv_dtype = lib.F32
    plain = h.mi355_attn_workspace_bytes(C.byref(p))
    p.sinks = addr
    assert h.mi355_attn_workspace_bytes(C.byref(p)) == plain
    assert (plain > (256 << 10)) == needs_scratch, plain            # (the blocks are what their names say: partials beyond the counters or not)
