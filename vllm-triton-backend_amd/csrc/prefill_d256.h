// What prefill_d256_kernel (prefill_d256.hip, 16-bit caches) and prefill_d256_fp8_kernel (prefill_d256_fp8.hip) share:
// the launch arguments, the accumulator-register map, the matrix instructions and the scalar block-table load.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace mi355 {

typedef __attribute__((ext_vector_type(4))) unsigned int du32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int du32x2_t;
typedef __attribute__((ext_vector_type(4))) float df32x4_t;
typedef __attribute__((ext_vector_type(4))) short ds16x4_t;

constexpr int kDRows = 128;                 // Q-block rows per workgroup
constexpr int kDTile = 64;                  // keys per tile
constexpr int kDAccO = 0, kDAccQ = 128;     // accumulator-register map
constexpr int kDORS = 256 * 2 + 16;         // padded row stride of the output rows parked in LDS (epilogue)
constexpr float kDLog2e = 1.4426950408889634f;
constexpr float kDDefer = 8.0f;             // log2 units a tile's maximum may exceed the row's reference by before it moves

struct D256Args {
  mi355_attn_params p;
  int group;        // G
  int block_q;      // tokens per Q block = 128 / G
  int page_shift;   // log2(page_size)
  uint32_t k_page_b, k_slot_b, v_page_b, v_slot_b;   // bytes between pages / key rows; validated < 2^32 on the host
  // key-split instantiations only (KS; grid.y = key_splits): workgroup (x, s) walks the s-th even share of its Q block's own
  // tile range and writes normalised partial rows / lse to p.out + s * out_split_stride / p.lse + s * lse_split_stride
  int key_splits;
  int64_t out_split_stride, lse_split_stride;        // elements
};

// The share of split `s` of a Q block's tile range [lo, hi) (prefill_mfma_kernel's rule: the host knows only the longest
// sequence, so every Q block deals its OWN tiles). Empty - lo == hi - where the range has fewer tiles than splits.
__device__ __forceinline__ void d_key_share(int& lo, int& hi, int s, int splits) {
  const int tps = (max(hi - lo, 0) + splits - 1) / splits;
  lo = min(lo + s * tps, hi);
  hi = min(hi, lo + tps);
}

template <typename F, int... I>
__device__ __forceinline__ void d_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void d_for(F&& f) { d_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{}); }

// The matrix instructions. asm volatile: they stay in source order, and the compiler neither pads nor counts anything
// around them - the wait states between them and ordinary code are written out where they are needed.
template <typename T> struct d256_ops;
#define MI355_DEF_D256_OPS(TAG, MFMA, CVT)                                                                          \
  template <> struct d256_ops<TAG> {                                                                               \
    /* S(VGPR) = K(VGPR) . Q'(AGPR) */                                                                              \
    template <int QA> static __device__ __forceinline__ void qk_zero(df32x4_t& s, const du32x4_t& k) {             \
      asm volatile(MFMA " %0, %1, a[%c2:%c3], 0" : "=&v"(s) : "v"(k), "n"(QA), "n"(QA + 3));                        \
    }                                                                                                              \
    /* S(VGPR) += K(VGPR) . Q'(AGPR) */                                                                             \
    template <int QA> static __device__ __forceinline__ void qk_acc(df32x4_t& s, const du32x4_t& k) {              \
      asm volatile(MFMA " %0, %1, a[%c2:%c3], %0" : "+v"(s) : "v"(k), "n"(QA), "n"(QA + 3));                        \
    }                                                                                                              \
    /* O(AGPR) += V(VGPR) . P(VGPR) */                                                                              \
    template <int OA> static __device__ __forceinline__ void pv(const du32x4_t& v, const du32x4_t& pf) {           \
      asm volatile(MFMA " a[%c2:%c3], %0, %1, a[%c2:%c3]" :: "v"(v), "v"(pf), "n"(OA), "n"(OA + 3));                \
    }                                                                                                              \
    static __device__ __forceinline__ uint32_t pack2(float lo, float hi) {                                         \
      uint32_t r; asm volatile(CVT " %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi)); return r;                           \
    }                                                                                                              \
  };
MI355_DEF_D256_OPS(bf16_t, "v_mfma_f32_16x16x32_bf16", "v_cvt_pk_bf16_f32")
MI355_DEF_D256_OPS(f16_t, "v_mfma_f32_16x16x32_f16", "v_cvt_pk_f16_f32")
#undef MI355_DEF_D256_OPS

template <int IDX> __device__ __forceinline__ void d_acc_write(uint32_t v) { asm volatile("v_accvgpr_write_b32 a%c0, %1" :: "n"(IDX), "v"(v)); }
template <int IDX> __device__ __forceinline__ float d_acc_read() { float r; asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(r) : "n"(IDX)); return r; }
// 2^x, pinned where it stands in the source (the wait state: a transcendental's result and the VALU instruction that reads it)
__device__ __forceinline__ float d_exp2(float x) { float r; asm volatile("v_exp_f32 %0, %1\n\ts_nop 0" : "=v"(r) : "v"(x)); return r; }

// One block-table entry through the scalar cache, in two halves: the load is started here and landed by d_sload_land(),
// which the caller places before the first use of `r` - and in the same loop iteration, so that no copy of `r` is made
// while it is in flight. `base` and `off` (bytes) are wave-uniform.
__device__ __forceinline__ void d_sload_start(int& r, const int32_t* base, int off) {
  const uint64_t b = (uint64_t)base;
  const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)b), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
  const uint64_t bu = ((uint64_t)bhi << 32) | blo;
  const int o = __builtin_amdgcn_readfirstlane(off);
  asm volatile("s_load_dword %0, %1, %2" : "=&s"(r) : "s"(bu), "s"(o) : "memory");
}
__device__ __forceinline__ void d_sload_land(int& r) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r) :: "memory"); }

int launch_prefill_d256_fp8(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks);   // prefill_d256_fp8.hip: an fp8 cache

}  // namespace mi355
