// decode_q8_kernel: split-KV decode attention at head size 128 with fp8 (e4m3) QUERIES over an fp8 cache (e4m3 / e5m2), with or
// without a sliding window and attention sinks, bf16 output (library 0.12.0). The arithmetic is prefill_q8_kernel's
// (prefill_q8.hip), so a row gets the same answer whichever of the two serves it; the work split is decode_splitkv_kernel's.
// Nothing is widened: K goes from HBM straight into the A operand of v_mfma_f32_16x16x128_f8f6f4, V through LDS only for its
// byte transpose.
//
// Work split: one WAVE per (sequence, KV head, split); no barriers, nothing shared between waves. The G <= 16 query heads of
// the KV head are the 16 B columns of S^T = K . Q^T (lane (i = lane & 15, g = lane >> 4) owns head i; columns G .. 15 are zero
// and never stored). A wave walks its split in tiles of 128 keys, the contraction length of O^T += V^T . P^T. Splits are whole
// tiles of the row's OWN key range (tiles of seq_len, from the window's first tile on): q8_range() is that arithmetic, shared
// by the kernel and the merge; a split past the row's last writes (m, l) = (-inf, 0) and no O.
//
//   Q   32 bytes a lane (head dims 32 g .. 32 g + 31 of head i), read once from global memory into 8 registers.
//   K   HBM -> VGPR -> MFMA, no LDS: lane (i, g) of key block kt holds the 32 bytes at dims 32 g .. of key row 16 kt + i - two
//       16-byte loads, four lanes covering one 128-byte row; 64 registers hold a tile. The NEXT tile's K is issued as soon as
//       S of this one is computed and is in flight under the softmax and the second product.
//   V   LDS-DMA on a scalar page base into the wave's private 16 KiB, 16 instructions of eight rows; read back with
//       ds_read_b64_tr_b8 under prefill_q8_kernel's XOR swizzle (chunk ^= ((row >> 1) & 3) | ((row >> 4) & 1) << 2, on the
//       per-lane SOURCE offset and again on the read address; tools/probes/ds_read_tr8.hip).
//   block table   four entries a tile (one per 32 keys: page size >= 32), fetched a tile ahead through the scalar cache.
//
// Data in flight - the choice: SINGLE-stage V with K as the prefetch, and MORE WAVES: 16 KiB of LDS a wave, a workgroup of four
// waves 64 KiB, two workgroups a CU (<= 256 registers a lane: two waves a SIMD). The next V tile is issued when the second
// product has read the current one, the next K tile before that; the kernel is memory-bound (26 matrix instructions and ~300
// vector ones per 32 KiB), so a wave spends most of a tile waiting with BOTH in flight: 8 waves x 32 KiB = 256 KiB a CU, twice
// what two-stage V at one wave a SIMD holds (4 x 32 KiB, 128 of the 160 KiB of LDS), and the second wave of a SIMD computes
// under the first one's wait. (That is what the map HOLDS; the split plan below fills half of it - 4 waves a CU measured faster
// than 8, profiles/r11/README.md.) LDS map: [wave 0 V tile | wave 1 | wave 2 | wave 3], 128 rows x 128 bytes each.
//
// Nothing outside the sequence reaches a sum: rows past it re-read its last row in K and V (valid data, never a stale 0x7f byte,
// no page beyond the sequence's last), and a masked score is -inf by select, whose P is exactly 0.
//
// Partials: slot ((seq Hq + hq) num_splits + split) of 128 + 32 floats - O without P's 2^8, then m (log2 domain), l - merged by
// decode_q8_merge_kernel in a second launch, which folds the sink exactly once; one split normalises and stores here.
#include <algorithm>
#include <cstdlib>

#include "prefill_d256.h"      // d_sload_start, the vector types, kDLog2e

namespace mi355 {

typedef __attribute__((ext_vector_type(8))) int zi32x8_t;
typedef __attribute__((ext_vector_type(2))) int zi32x2_t;
typedef __attribute__((ext_vector_type(2))) float zf32x2_t;

constexpr int kZTile = 128;                  // keys per tile
constexpr int kZRowB = 128;                  // bytes per key row
constexpr int kZTileB = kZTile * kZRowB;     // 16 KiB: a wave's V tile
constexpr int kZWaves = 4;
constexpr int kZLds = kZWaves * kZTileB;
constexpr int kZSlot = 128 + 32;             // floats per partial: O, m, l, padding to a 128-byte multiple
constexpr int kZMaxSplits = 128;             // what num_segments may ask for
constexpr int kZPlanSplits = 32;             // what the library's own plan stops at
constexpr size_t kZCounterRegion = (size_t)256 << 10;   // head of every workspace (include/mi355_attn.h); not used here, never written
constexpr float kZPShift = 8.0f;             // P = 2^8 exp(s - m)
constexpr float kZPInv = 0.00390625f;
static_assert(kZLds == 64 * 1024 && 2 * kZLds <= 160 * 1024, "decode_q8_kernel: LDS map (two workgroups a CU)");
static_assert((kZSlot * sizeof(float)) % 128 == 0, "decode_q8_kernel: partial slots are 128-byte multiples");

struct DecodeQ8Args {
  mi355_attn_params p;
  float* slots;     // split partials (null with one split)
  int num_splits;
  int group;        // G
  int page_shift;   // log2(page_size)
  uint32_t k_page_b, k_slot_b, v_page_b, v_slot_b;   // bytes between pages / key rows; validated < 2^32 on the host
};

// The tiles of a one-token row of `seq_len` keys and how `num_splits` splits share them.
struct Q8Range { int tile_lo, tile_hi, tps, active; };
__device__ __forceinline__ Q8Range q8_range(int seq_len, int sw, int num_splits) {
  Q8Range r;
  r.tile_lo = sw > 0 ? max(0, seq_len - sw) / kZTile : 0;
  r.tile_hi = (max(seq_len, 0) + kZTile - 1) / kZTile;
  const int n = max(0, r.tile_hi - r.tile_lo);
  r.tps = max(1, (n + num_splits - 1) / num_splits);
  r.active = (n + r.tps - 1) / r.tps;
  return r;
}

template <bool E5>
__device__ __forceinline__ df32x4_t z_mfma(const zi32x8_t& a, const zi32x8_t& b, const df32x4_t& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, E5 ? 1 : 0, 0, 0, 0, 0, 0);
}

template <bool E5, bool SPLIT>
__global__ __launch_bounds__(256, 2) void decode_q8_kernel(const DecodeQ8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const mi355_attn_params& p = a.p;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = a.group;
  // work item: split fastest, then KV head, then sequence (every sequence has one query token: token == sequence)
  const int item = (int)blockIdx.x * kZWaves + wave;
  if (item >= p.num_seqs * p.num_kv_heads * a.num_splits) return;
  const int split = item % a.num_splits;
  const int head = (item / a.num_splits) % p.num_kv_heads;
  const int seq = item / a.num_splits / p.num_kv_heads;
  const int seq_len = p.seqused_k[seq];
  const int sw = p.sliding_window;
  const Q8Range rg = q8_range(seq_len, sw, a.num_splits);
  const bool live = split < rg.active;
  const int t_lo = live ? rg.tile_lo + split * rg.tps : 0;
  const int t_hi = live ? min(t_lo + rg.tps, rg.tile_hi) : 0;
  const int lim = seq_len - 1;                             // the row sees keys lo_key .. lim
  const int lo_key = sw > 0 ? seq_len - sw : 0;

  const int r16 = lane & 15, g4 = lane >> 4;
  const bool col_ok = r16 < G;
  const int hq = head * G + min(r16, G - 1);

  // ---- scores are c * (q . k): |c| rides the exponent's FMA, its sign the queries ----
  const float c_signed = p.scale * kDLog2e * (p.k_scale ? p.k_scale[0] : 1.0f);
  const float c2 = fmaxf(fabsf(c_signed), 1.17549435e-38f);      // (never 0: a masked score's -inf times c stays -inf)
  const uint32_t q_flip = c_signed < 0.0f ? 0x80808080u : 0u;
  const float v_sc = p.v_scale ? p.v_scale[0] : 1.0f;

  // ---- Q: 32 bytes of the lane's head, dims 32 g4 .. + 31; a column past the group is zero ----
  zi32x8_t qf;
  {
    const char* qp = (const char*)p.q + (int64_t)seq * p.q_stride_token + (int64_t)hq * p.q_stride_head + 32 * g4;
    const du32x4_t lo = *(const du32x4_t*)qp, hi = *(const du32x4_t*)(qp + 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qf[j] = col_ok ? (int)(lo[j] ^ q_flip) : 0;
      qf[4 + j] = col_ok ? (int)(hi[j] ^ q_flip) : 0;
    }
  }

  const int32_t* bt = p.block_table + (int64_t)seq * p.block_table_stride;
  const char* kbase = (const char*)p.k_cache + (int64_t)head * p.k_stride_head;
  const char* vbase = (const char*)p.v_cache + (int64_t)head * p.v_stride_head;
  const int last_group = (max(seq_len, 1) - 1) >> 5;
  const int page_mask = p.page_size - 1;
  const uint32_t lds0 = lds_addr(smem) + (uint32_t)(wave * kZTileB);
  const char* st = smem + wave * kZTileB;
  // 32-key group j of a tile: inside one page, and never past the sequence's last group
  auto group_of = [&](int tile, int j) { return min(tile * 4 + j, last_group); };
  auto entry_off = [&](int tile, int j) { return ((group_of(tile, j) << 5) >> a.page_shift) << 2; };

  // K of a tile into registers: key block kt = 2 j + h is rows 16 h .. 16 h + 15 of group j; rows past the sequence's last re-read it
  auto issue_k = [&](int tile, int pg0, int pg1, int pg2, int pg3, zi32x8_t (&kf)[8]) {
    const int pg[4] = {pg0, pg1, pg2, pg3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key0 = group_of(tile, j) << 5;
      const int maxr = seq_len - 1 - key0;
      const char* kb = kbase + ((uint64_t)(uint32_t)pg[j] * a.k_page_b + (uint64_t)(uint32_t)(key0 & page_mask) * a.k_slot_b);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const char* kp = kb + (uint32_t)(min(16 * h + r16, maxr) * (int)a.k_slot_b + 32 * g4);
        const du32x4_t lo = *(const du32x4_t*)kp, hi = *(const du32x4_t*)(kp + 16);
        kf[2 * j + h] = zi32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      }
    }
  };
  // V of a tile into the wave's LDS: instruction i of group j lands rows 32 j + 8 i + (lane >> 3), chunk position lane & 7 holding
  // logical chunk position ^ f(row) (f of the tile row 32 j + R is f of R)
  auto issue_v = [&](int tile, int pg0, int pg1, int pg2, int pg3) {
    const int pg[4] = {pg0, pg1, pg2, pg3};
    const int c8 = lane & 7;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key0 = group_of(tile, j) << 5;
      const int maxr = seq_len - 1 - key0;
      const uint64_t vb = (uint64_t)vbase + (uint64_t)(uint32_t)pg[j] * a.v_page_b + (uint64_t)(uint32_t)(key0 & page_mask) * a.v_slot_b;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int R = 8 * i + (lane >> 3);
        glds16_s((uint32_t)(min(R, maxr) * (int)a.v_slot_b + ((c8 ^ (((R >> 1) & 3) | (((R >> 4) & 1) << 2))) << 4)), vb, lds0 + j * (32 * kZRowB) + i * 1024);
      }
    }
  };

  // V read (db, c): lane pair r8 of the quarter wave addresses key row 32 c + vrow, logical chunk db, its half r16 & 1 -> v_rd[db] + 4096 c
  const int r8 = r16 >> 1, vrow = 16 * (r8 >> 2) + 4 * g4 + (r8 & 3);
  int v_rd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v_rd[j] = vrow * kZRowB + ((j ^ (((vrow >> 1) & 3) | (((vrow >> 4) & 1) << 2))) << 4) + 8 * (r16 & 1);

  // O^T [128 dims x 16 heads] and the row sums: lane (r16, g4) register r of block db <-> head r16, dim 16 db + 4 g4 + r
  df32x4_t o[8], l_acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int db = 0; db < 8; ++db) o[db] = df32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
  float m_run = -INFINITY;                                 // running maximum of the raw scores q . k
  const int one4 = E5 ? 0x3c3c3c3c : 0x38383838;           // 1.0 four times, in the cache's format
  const zi32x8_t ones = {one4, one4, one4, one4, one4, one4, one4, one4};

  zi32x8_t kf[8];
  if (t_lo < t_hi) {
    int e0, e1, e2, e3;
    d_sload_start(e0, bt, entry_off(t_lo, 0)); d_sload_start(e1, bt, entry_off(t_lo, 1));
    d_sload_start(e2, bt, entry_off(t_lo, 2)); d_sload_start(e3, bt, entry_off(t_lo, 3));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(e0), "+s"(e1), "+s"(e2), "+s"(e3) :: "memory");
    issue_k(t_lo, e0, e1, e2, e3, kf);
    issue_v(t_lo, e0, e1, e2, e3);
  }

  for (int tile = t_lo; tile < t_hi; ++tile) {
    const bool has_next = tile + 1 < t_hi;
    // the next tile's pages (SGPRs): started and landed in this same iteration, on every iteration (the split's last tile asks
    // for its own again) so that no branch joins a register whose load is in flight
    const int nt = min(tile + 1, t_hi - 1);
    int n0, n1, n2, n3;
    d_sload_start(n0, bt, entry_off(nt, 0)); d_sload_start(n1, bt, entry_off(nt, 1));
    d_sload_start(n2, bt, entry_off(nt, 2)); d_sload_start(n3, bt, entry_off(nt, 3));
    glds_wait_all();                                       // this tile's K (registers) and V (LDS) have landed
    const int key_base = tile * kZTile;

    // ---- S^T = K . Q^T: one instruction per key block; then the registers take the next tile's K ----
    df32x4_t s[8];
    const df32x4_t zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) s[kt] = z_mfma<E5>(kf[kt], qf, zero);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(n0), "+s"(n1), "+s"(n2), "+s"(n3) :: "memory");
    if (has_next) issue_k(tile + 1, n0, n1, n2, n3, kf);

    // ---- softmax on the raw scores: register r of key block kt <-> key key_base + 16 kt + 4 g4 + r ----
    if (key_base + kZTile > seq_len || key_base < lo_key) {
#pragma unroll
      for (int kt = 0; kt < 8; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key_base + 16 * kt + 4 * g4 + r;
          s[kt][r] = (key <= lim && key >= lo_key) ? s[kt][r] : -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      mx = fmaxf(fmaxf(mx, s[kt][0]), s[kt][1]);
      mx = fmaxf(fmaxf(mx, s[kt][2]), s[kt][3]);
    }
    mx = fmaxf(mx, lane_xor16(mx));                        // the other three quarter waves hold the head's other keys
    mx = fmaxf(mx, lane_xor32(mx));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new > -INFINITY ? m_new : 0.0f;
    const float alpha = (m_new == m_run || !(m_run > -INFINITY)) ? 1.0f : __builtin_amdgcn_exp2f((m_run - m_use) * c2);
    m_run = m_new;
    const float off = kZPShift - m_use * c2;
    zi32x8_t pf, pl;                                       // P = pf + pl: the rounded weights and their rounded residuals
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][0], c2, off)), e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][1], c2, off));
      const float e2 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][2], c2, off)), e3 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][3], c2, off));
      const int hi = __builtin_amdgcn_cvt_pk_fp8_f32(e2, e3, __builtin_amdgcn_cvt_pk_fp8_f32(e0, e1, 0, false), true);
      const zf32x2_t h01 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), h23 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
      pf[kt] = hi;
      pl[kt] = __builtin_amdgcn_cvt_pk_fp8_f32(e2 - h23[0], e3 - h23[1], __builtin_amdgcn_cvt_pk_fp8_f32(e0 - h01[0], e1 - h01[1], 0, false), true);
    }
    if (!__all(alpha == 1.0f)) {                           // O^T = alpha O^T and l = alpha l, only when some head's maximum moved
      l_acc *= alpha;
#pragma unroll
      for (int db = 0; db < 8; ++db) o[db] *= alpha;
    }
    // ---- O^T += V^T . P^T: four transposed reads make the operand of one dim block ----
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      zi32x8_t vf;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const zi32x2_t v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) zi32x2_t*)(st + v_rd[db] + 4096 * c));
        vf[2 * c] = v[0];
        vf[2 * c + 1] = v[1];
      }
      o[db] = z_mfma<E5>(vf, pf, o[db]);
      o[db] = z_mfma<E5>(vf, pl, o[db]);
    }
    l_acc = z_mfma<E5>(ones, pf, l_acc);
    l_acc = z_mfma<E5>(ones, pl, l_acc);
    if (has_next) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every read of this tile's V has returned: its LDS takes the next one
      issue_v(tile + 1, n0, n1, n2, n3);
    }
  }

  // ---- (m, l) in the log2 domain of the scaled scores, l and O without P's factor ----
  float l = l_acc[0] * kZPInv, m = m_run > -INFINITY ? m_run * c2 : -INFINITY;
  if (SPLIT) {
    if (!col_ok) return;
    float* slot = a.slots + (((int64_t)seq * p.num_q_heads + hq) * a.num_splits + split) * kZSlot;
    if (live) {
#pragma unroll
      for (int db = 0; db < 8; ++db) *(df32x4_t*)(slot + 16 * db + 4 * g4) = o[db] * kZPInv;
    }
    if (g4 == 0) *(zf32x2_t*)(slot + 128) = zf32x2_t{m, l};
    return;
  }
  const float sink_w = (p.sinks && col_ok) ? fold_sink<true>(m, l, p.sinks[hq]) : 1.0f;   // one split: the row's (m, l) is final here
  if (!col_ok) return;
  if (p.lse && g4 == 0) p.lse[(int64_t)seq * p.lse_stride_token + hq] = l > 0.0f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : -INFINITY;
  const float inv = l > 0.0f ? v_sc * sink_w * kZPInv / l : 0.0f;      // (V was summed unscaled, P times 2^8)
  uint16_t* op = (uint16_t*)p.out + (int64_t)seq * p.out_stride_token + (int64_t)hq * p.out_stride_head + 4 * g4;
#pragma unroll
  for (int db = 0; db < 8; ++db)
    *(du32x2_t*)(op + 16 * db) = du32x2_t{pack_bf16x2(o[db][0] * inv, o[db][1] * inv), pack_bf16x2(o[db][2] * inv, o[db][3] * inv)};
}

// The merge of a row's split partials: one wave per (sequence, query head), two output columns a lane. The partials of eight
// splits are loaded before the first is folded, so a row of up to eight splits is one memory round trip.
__global__ __launch_bounds__(64) void decode_q8_merge_kernel(const DecodeQ8Args a) {
  const mi355_attn_params& p = a.p;
  const int seq = blockIdx.x, hq = blockIdx.y, lane = threadIdx.x;
  const int active = q8_range(p.seqused_k[seq], p.sliding_window, a.num_splits).active;
  const float* slot0 = a.slots + ((int64_t)seq * p.num_q_heads + hq) * a.num_splits * kZSlot;
  float m_all = -INFINITY;
  for (int s = 0; s < active; ++s) m_all = fmaxf(m_all, slot0[s * kZSlot + 128]);
  float l_all = 0.0f;
  zf32x2_t acc = {0.0f, 0.0f};
  for (int s0 = 0; s0 < active; s0 += 8) {
    zf32x2_t ml[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float* slot = slot0 + min(s0 + i, active - 1) * kZSlot;     // a row past `active` re-reads the last with weight 0
      ml[i] = *(const zf32x2_t*)(slot + 128);
      v[i] = ((const zf32x2_t*)slot)[lane];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float w = (s0 + i < active && ml[i][0] > -INFINITY) ? __builtin_amdgcn_exp2f(ml[i][0] - m_all) : 0.0f;
      l_all += ml[i][1] * w;
      acc += v[i] * w;
    }
  }
  const float sink_w = p.sinks ? fold_sink<true>(m_all, l_all, p.sinks[hq]) : 1.0f;      // the partials are sink-free: folded once, here
  const float inv = l_all > 0.0f ? (p.v_scale ? p.v_scale[0] : 1.0f) * sink_w / l_all : 0.0f;
  if (p.lse && lane == 0) p.lse[(int64_t)seq * p.lse_stride_token + hq] = l_all > 0.0f ? (m_all + __builtin_amdgcn_logf(l_all)) * 0.6931471805599453f : -INFINITY;
  uint32_t* op = (uint32_t*)((uint16_t*)p.out + (int64_t)seq * p.out_stride_token + (int64_t)hq * p.out_stride_head);
  op[lane] = pack_bf16x2(acc[0] * inv, acc[1] * inv);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The steps this family takes, beyond what prefill_q8_supported() asks of every call with fp8 queries: a pure decode step under
// MI355_SELECT_AUTO with at most 16 query heads per KV head. Host arithmetic only.
bool decode_q8_step(const mi355_attn_params& p) {
  return (p.q_dtype == MI355_FP8_E4M3 || p.q_dtype == MI355_FP8_E5M2) && p.kernel_select == MI355_SELECT_AUTO && p.max_seqlen_q == 1 &&
         p.num_tokens == p.num_seqs && !p.skip_decodes && !p.only_decodes && p.num_kv_heads > 0 && p.num_q_heads / p.num_kv_heads <= 16;
}

// Capture-stable split count: host-known sizes only (sequences, KV heads, max_seqlen_k).
static int plan_q8_splits(const mi355_attn_params& p) {
  const int max_tiles = (p.max_seqlen_k + kZTile - 1) / kZTile;
  if (max_tiles <= 1) return 1;      // one tile, or no bound given (max_seqlen_k == 0): one split walks every row to its own length
  int want = p.num_segments;
  if (want <= 0) {
    // Waves in flight: 4 a CU, half of what the LDS map holds, and at most 32 splits - from the sweep in profiles/r11/README.md
    // (graph replay, e4m3): 16 x 32768 keys, Hk 8: 8 splits 231 us, 16: 247, 32: 250; 64 x 8192: 1 split 244 us, 2: 200, 4: 232,
    // 8: 241; batch 1 at 32768 keys: 16 splits 52.9 us, 32: 36.0, 128: 43.4 (the merge walks a row's partials eight at a
    // time); at 8192 keys: 16: 19.5, 32: 18.3, 64: 22.0. MI355_DECODE_Q8_TARGET_WAVES overrides the number for sweeps.
    static const long target_env = [] { const char* e = lab_env("MI355_DECODE_Q8_TARGET_WAVES"); return e ? atol(e) : 0L; }();
    const long target = target_env > 0 ? target_env : 256L * 4;
    const long base = std::max(1L, (long)p.num_seqs * p.num_kv_heads);      // waves with one split each
    want = (int)std::min<long>((target + base - 1) / base, kZPlanSplits);
  }
  want = std::max(1, std::min(want, std::min(max_tiles, kZMaxSplits)));
  const int tps = (max_tiles + want - 1) / want;
  return std::max(1, (max_tiles + tps - 1) / tps);
}

size_t decode_q8_workspace_bytes(const mi355_attn_params& p) {
  const int splits = plan_q8_splits(p);
  if (splits <= 1) return 0;
  return kZCounterRegion + (size_t)p.num_seqs * p.num_q_heads * splits * kZSlot * sizeof(float);
}

template <bool E5, bool SPLIT>
static int launch_decode_q8_t(const DecodeQ8Args& a, hipStream_t stream) {
  const mi355_attn_params& p = a.p;
  static std::atomic<uint64_t> lds_opt_in{0};
  const int rc0 = ensure_dynamic_lds((const void*)decode_q8_kernel<E5, SPLIT>, kZLds, lds_opt_in, "hipFuncSetAttribute(decode_q8)");
  if (rc0 != MI355_OK) return rc0;
  const long items = (long)p.num_seqs * p.num_kv_heads * a.num_splits;
  hipLaunchKernelGGL((decode_q8_kernel<E5, SPLIT>), dim3((unsigned)((items + kZWaves - 1) / kZWaves)), dim3(kZWaves * 64), kZLds, stream, a);
  int rc = check_hip(hipGetLastError(), "decode_q8_kernel launch");
  if (rc == MI355_OK && SPLIT) {
    hipLaunchKernelGGL(decode_q8_merge_kernel, dim3(p.num_seqs, p.num_q_heads), dim3(64), 0, stream, a);
    rc = check_hip(hipGetLastError(), "decode_q8_merge_kernel launch");
  }
  if (rc == MI355_OK) set_kernel_name(SPLIT ? "decode_splitkv_q8" : "decode_single_q8");
  return rc;
}

// A validated decode_q8_step(). Without the workspace its plan asks for (a caller written against 0.11.0 passes none) the step
// runs on prefill_q8_kernel as it did then.
int launch_decode_q8(const mi355_attn_params& p, void* ws, size_t ws_bytes, hipStream_t stream) {
  const size_t need = decode_q8_workspace_bytes(p);
  if (need > 0 && (!ws || ws_bytes < need)) {
    mi355_attn_params q = p;
    q.num_segments = 0;
    return launch_prefill_q8(q, stream);
  }
  DecodeQ8Args a;
  a.p = p;
  a.num_splits = plan_q8_splits(p);
  a.slots = need ? (float*)((char*)ws + kZCounterRegion) : nullptr;
  a.group = p.num_q_heads / p.num_kv_heads;
  a.page_shift = __builtin_ctz((unsigned)p.page_size);
  a.k_page_b = (uint32_t)p.k_stride_page; a.k_slot_b = (uint32_t)p.k_stride_slot;      // one byte an element
  a.v_page_b = (uint32_t)p.v_stride_page; a.v_slot_b = (uint32_t)p.v_stride_slot;
  const bool e5 = p.kv_dtype == MI355_FP8_E5M2;
  if (a.num_splits > 1) return e5 ? launch_decode_q8_t<true, true>(a, stream) : launch_decode_q8_t<false, true>(a, stream);
  return e5 ? launch_decode_q8_t<true, false>(a, stream) : launch_decode_q8_t<false, false>(a, stream);
}

}  // namespace mi355
