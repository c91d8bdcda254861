"""CPU-only: the host side of split-KV decode with fp8 queries (library 0.12.0, csrc/decode_q8.hip) through the C ABI with dummy
aligned addresses (nothing is read): which steps get a split plan and how large its workspace is."""

import ctypes as C
import threading

import pytest

from test_cpu_sinks import _params as _bf16_params, addr, lib  # noqa: F401  (the fixtures and the Hq 32 / Hk 8 / D 128 block)

COUNTERS = 256 << 10
SLOT_ROW = 64 * 32 * (128 + 32) * 4            # one split of every (sequence, query head): 128 + 32 floats each


def _params(lib, addr):
    """The decode block: 64 sequences of one e4m3 query token, up to 8192 keys in an e4m3 flash-layout cache of 32-slot pages."""
    p = _bf16_params(lib, addr, 64, 64, 1, 8192)
    p.q_dtype = p.kv_dtype = lib.FP8_E4M3
    p.page_size, p.k_stride_page, p.v_stride_page = 32, 32768, 32768
    return p


def test_the_decode_block_gets_a_split_plan(lib, addr):
    h, p = lib.load(), _params(lib, addr)
    n = h.mi355_attn_workspace_bytes(C.byref(p))
    assert n > COUNTERS and (n - COUNTERS) % SLOT_ROW == 0, n
    assert h.mi355_decode_write_fusable(C.byref(p)) == 0
    p.num_segments = 4
    assert h.mi355_attn_workspace_bytes(C.byref(p)) == COUNTERS + 4 * SLOT_ROW
    assert h.mi355_decode_write_fusable(C.byref(p)) == 0


@pytest.mark.parametrize("change", [dict(max_seqlen_k=128), dict(max_seqlen_k=0), dict(max_seqlen_k=0, num_segments=4), dict(kernel_select=2),
                                    dict(num_kv_heads=1), dict(only_decodes=1), dict(max_seqlen_q=2)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_everything_else_keeps_a_workspace_of_zero(lib, addr, change):
    """One tile, no key bound given (one split walks each row to its own length, whatever num_segments asks), the Q-block kernel by
    selection, G = 32, a decode launch of a mixed step, a step that is no decode step."""
    h, p = lib.load(), _params(lib, addr)
    for k, v in change.items():
        setattr(p, k, v)
    if "num_kv_heads" in change:
        p.k_stride_slot = p.v_stride_slot = 128
        p.k_stride_page = p.v_stride_page = 4096
    assert h.mi355_attn_workspace_bytes(C.byref(p)) == 0 and h.mi355_decode_write_fusable(C.byref(p)) == 0


def test_select_3d_is_still_refused_by_name(lib, addr):
    """On a thread of its own: the library keeps its last error message per thread, and test_cpu_host.py, which runs after this
    file, expects none on the main thread."""
    seen = []

    def body():
        h, p = lib.load(), _params(lib, addr)
        p.kernel_select = 3
        seen.append((h.mi355_attn_workspace_bytes(C.byref(p)), h.mi355_decode_write_fusable(C.byref(p)),
                     h.mi355_unified_attention(C.byref(p), None, 0, None), lib.last_error()))

    t = threading.Thread(target=body)
    t.start()
    t.join()
    nbytes, fusable, rc, message = seen[0]
    assert nbytes == 0 and fusable == 0 and rc == lib.MI355_ERR_UNSUPPORTED
    assert "MI355_SELECT_3D" in message, message
