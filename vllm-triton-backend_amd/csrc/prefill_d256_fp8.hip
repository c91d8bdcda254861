// prefill_d256_fp8_kernel: causal prefill attention at head size 256 over an fp8 cache (bf16 / f16 queries, e4m3 / e5m2 cache,
// with or without a sliding window). prefill_d256_kernel's (prefill_d256.hip) work split, softmax and epilogue - four waves of
// 32 query rows, O and Q' in accumulator registers that only the asm statements name, tiles of 64 keys by LDS-DMA - on a data
// path of its own: the cache stays fp8 from HBM through LDS into registers and is widened THERE, by the packed converts
// (v_cvt_scalef32_pk_{bf16,f16}_{fp8,bf8} at scale 1.0: exact), straight into the matrix instruction. No LDS store, no staging
// registers; k_scale rides in Q', v_scale in the epilogue's 1 / l.
//
// LDS: two stages of [K tile 16 KiB | V tile 16 KiB]; a row is 256 bytes = 16 chunks of 16 bytes, unpadded. An LDS-DMA
// instruction writes four rows; wave w stages rows 16 w .. 16 w + 15 of a tile with four instructions for K and four for V
// (one block-table entry per wave and tile, a tile ahead, through the scalar cache). Rows of 256 bytes all start on bank 0, so
// the chunk index is XORed on the per-lane SOURCE offset and again on the read address:
//   K (ds_read_b128: a quarter wave reads rows 16 kt + 0 .. 15 at one chunk):          chunk ^= row & 15
//   V (ds_read_b64_tr_b8: a half wave reads the sixteen rows 32 c + {0 .. 7, 16 .. 23} (or {8 .. 15, 24 .. 31}) at one chunk,
//      two lanes a row):                                                                chunk ^= (row & 7) | ((row & 16) >> 1)
// Both give sixteen different chunks = all banks once per quarter / half wave.
//
// K operand (A of S^T = K . Q'^T, 16 keys x 32 dims): lane (q = lane & 15, g = lane >> 4) reads chunk 4 kp + g of key row
// 16 kt + q: dims 64 kp + 16 g .. + 15. Bytes 0 .. 7 widen to the fragment of k-step 2 kp, bytes 8 .. 15 to that of 2 kp + 1: k-slot e
// of lane group g in k-step ks is head dim 64 (ks >> 1) + 16 g + 8 (ks & 1) + e, and Q' is written into a[128 ..] in the same
// order (a contraction does not care). 16 reads and 128 converts feed a tile's 64 matrix instructions.
//
// V operand (A of O^T += V^T . P^T, 16 dims x 32 keys): ds_read_b64_tr_b8 transposes an [8][16] byte matrix inside a quarter
// wave - lane j receives byte j of the eight 16-byte rows that lanes (2 r, 2 r + 1) address, r = 0 .. 7 (tools/probes/
// ds_read_tr8.hip). Lane pair r of quarter g addresses key 32 c + 16 (r >> 2) + 4 g + (r & 3) at columns 16 db .. + 15, so k-slot e
// of k-step c is key 32 c + 16 (e >> 2) + 4 g + (e & 3): the order in which the lane's S registers are packed into P, the
// 16-bit form's. ONE read and four converts per fragment; 32 reads and 128 converts feed a tile's 64 matrix instructions.
//
// The converts are asm volatile like the matrix instructions, two behind each: fragment m's first matrix instruction, the
// second half of fragment m + 1, fragment m's second matrix instruction, the first half of fragment m + 2. A wave issues in
// order, so two converts (8 cycles) fit in the 12 cycles a matrix instruction leaves free, where four in a row would hold the
// next one back; and a matrix instruction always stands between a VALU-written operand and the one that reads it.
//
// Nothing outside the sequence reaches a sum: rows past it re-read its last row (valid fp8 data, never a stale 0x7f byte), and
// a masked score is -inf, whose P is exactly 0.
//
// Key-split form (KS, library 0.13.0): as prefill_d256_kernel's - grid.y = splits, an even share of the Q block's own tile
// range, partial rows (v_scale applied) and lse to the workspace buffers of split s.
#include <cstdlib>

#include "prefill_d256.h"

namespace mi355 {

typedef __attribute__((ext_vector_type(2))) int di32x2_t;

constexpr int kFRowB = 256;                 // bytes per key row
constexpr int kFTileB = kDTile * kFRowB;    // 16 KiB: one K or V tile
constexpr int kFStageB = 2 * kFTileB;       // K tile then V tile
constexpr int kFOutB = 4 * 32 * kDORS;      // the epilogue parks the output rows in LDS
constexpr int kFLds = 2 * kFStageB > kFOutB ? 2 * kFStageB : kFOutB;
static_assert(kFLds <= 160 * 1024, "prefill_d256_fp8_kernel: LDS map");

// Four fp8 bytes (one word) -> half a matrix operand: four 16-bit values in byte order, two packed words.
template <typename T, typename KVT> struct d256_widen;
#define MI355_DEF_D256_WIDEN(TAG, KV, CVT)                                                                \
  template <> struct d256_widen<TAG, KV> {                                                               \
    static __device__ __forceinline__ void half(uint32_t& x0, uint32_t& x1, uint32_t a) {                \
      asm volatile(CVT " %0, %1, 1.0" : "=v"(x0) : "v"(a));                                               \
      asm volatile(CVT " %0, %1, 1.0 op_sel:[1,0,0]" : "=v"(x1) : "v"(a));                                \
    }                                                                                                    \
  };
MI355_DEF_D256_WIDEN(bf16_t, e4m3_t, "v_cvt_scalef32_pk_bf16_fp8")
MI355_DEF_D256_WIDEN(bf16_t, e5m2_t, "v_cvt_scalef32_pk_bf16_bf8")
MI355_DEF_D256_WIDEN(f16_t, e4m3_t, "v_cvt_scalef32_pk_f16_fp8")
MI355_DEF_D256_WIDEN(f16_t, e5m2_t, "v_cvt_scalef32_pk_f16_bf8")
#undef MI355_DEF_D256_WIDEN

template <typename T, typename KVT, bool SW, bool KS>
__global__ __launch_bounds__(256, 1) void prefill_d256_fp8_kernel(const D256Args a) {
  using ops = d256_ops<T>;
  using wid = d256_widen<T, KVT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  asm volatile("" ::: "a255");                 // the kernel owns all 256 accumulator registers

  const mi355_attn_params& p = a.p;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = a.group, BQ = a.block_q;

  // 1-D grid, KV head fastest, heaviest Q blocks first (prefill_d256_kernel)
  const int nqb = (int)(gridDim.x / p.num_kv_heads);
  const int head = (int)(blockIdx.x % p.num_kv_heads);
  const int qblock = nqb - 1 - (int)(blockIdx.x / p.num_kv_heads);
  int q_start, q_len, seq_len;
  const int seq = find_seq_and_lengths(p.cu_seqlens_q, p.seqused_k, p.num_seqs, qblock, BQ, lane, q_start, q_len, seq_len);
  if (seq < 0) return;
  const int qb_local = qblock - (q_start / BQ + seq);
  if (qb_local * BQ >= q_len) return;                      // surplus Q block
  if (q_len <= p.skip_decodes) return;                     // rows of another launch
  if (p.only_decodes && q_len > p.only_decodes) return;
  const int ctx_len = seq_len - q_len;
  const int tok0 = qb_local * BQ;                          // first query token (inside the sequence's query) of this Q block
  const int sw = SW ? p.sliding_window : 0;

  // ---- this lane's two query rows: 32 wave + 16 rb + (lane & 15) ---------------------------------
  const int r16 = lane & 15, g4 = lane >> 4;
  int tok_local[2], hq[2], lim[2], lo_key[2];
  bool row_ok[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int m_row = wave * 32 + 16 * rb + r16;
    tok_local[rb] = tok0 + m_row / G;
    hq[rb] = head * G + m_row % G;
    row_ok[rb] = (m_row < BQ * G) && (tok_local[rb] < q_len);
    const int q_abs = ctx_len + tok_local[rb];             // the row sees keys lo_key .. lim
    lim[rb] = row_ok[rb] ? min(q_abs, seq_len - 1) : -1;
    lo_key[rb] = SW ? q_abs - sw + 1 : 0;
  }
  // wave-uniform bounds of the rows this wave / workgroup owns
  const int w_tok_lo = tok0 + (wave * 32) / G;
  const int w_tok_hi = min(min(tok0 + (wave * 32 + 31) / G, tok0 + BQ - 1), q_len - 1);
  const int wg_tok_hi = min(tok0 + BQ - 1, q_len - 1);
  const int n_keys_wg = max(min(ctx_len + wg_tok_hi + 1, seq_len), 0);
  const int wave_keys = min(ctx_len + w_tok_hi + 1, seq_len);
  const bool wave_has_rows = w_tok_lo <= w_tok_hi;
  const int wave_first_key = SW ? ctx_len + w_tok_lo - sw + 1 : 0;       // no row of the wave sees a key below
  int tile_lo = SW ? max(0, ctx_len + tok0 - sw + 1) / kDTile : 0;
  int tile_hi = (n_keys_wg + kDTile - 1) / kDTile;
  // key-split launch: this workgroup's share of those tiles - possibly none, it then writes 0 / -inf, which the merge weighs
  // with 0. Masks and the tail clamp are functions of absolute key positions, the pipeline's parity of tile - tile_lo.
  const int ksplit = KS ? (int)blockIdx.y : 0;
  if constexpr (KS) d_key_share(tile_lo, tile_hi, ksplit, a.key_splits);

  // ---- Q' = Q * scale * log2(e) * k_scale into a[128 ..]: lane (r16, g4) holds, for k-step ks, the head dims
  //      64 (ks >> 1) + 16 g4 + 8 (ks & 1) .. + 7 - the order in which a 16-byte fp8 read of K delivers two k-steps ----
  const float scale2 = p.scale * kDLog2e * (p.k_scale ? p.k_scale[0] : 1.0f);
  const float v_sc = p.v_scale ? p.v_scale[0] : 1.0f;
  // (a row outside the Q block reads the sequence's last query token instead - always a valid address - and is scaled by 0)
  {
    du32x4_t qv[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const uint16_t* qp = (const uint16_t*)p.q + (int64_t)(q_start + min(tok_local[rb], q_len - 1)) * p.q_stride_token + (int64_t)hq[rb] * p.q_stride_head + 16 * g4;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qv[rb][ks] = *(const du32x4_t*)(qp + 64 * (ks >> 1) + 8 * (ks & 1));
    }
    d_for<64>([&](auto I) __attribute__((always_inline)) {
      constexpr int i = decltype(I)::value, rb = i >> 5, ks = (i >> 2) & 7, e = i & 3;
      const uint32_t w = qv[rb][ks][e];
      const float sc = row_ok[rb] ? scale2 : 0.0f;
      float x0, x1;
      if constexpr (__is_same(T, bf16_t)) { x0 = bits_to_f32(w << 16); x1 = bits_to_f32(w & 0xffff0000u); }
      else { x0 = f16_to_f32((uint16_t)w); x1 = f16_to_f32((uint16_t)(w >> 16)); }
      d_acc_write<kDAccQ + i>(ops::pack2(x0 * sc, x1 * sc));
    });
  }
  d_for<128>([&](auto I) __attribute__((always_inline)) { d_acc_write<kDAccO + decltype(I)::value>(0u); });

  // ---- LDS-DMA: wave w stages key rows 16 w .. 16 w + 15 of a tile, four rows per instruction ------------------
  // instruction i: LDS row R = 4 i + (lane >> 4), chunk position lane & 15 holds logical chunk position ^ f(16 w + R)
  const int32_t* bt = p.block_table + (int64_t)seq * p.block_table_stride;
  const char* kbase = (const char*)p.k_cache + (int64_t)head * p.k_stride_head;
  const char* vbase = (const char*)p.v_cache + (int64_t)head * p.v_stride_head;
  const int last_group = (max(seq_len, 1) - 1) >> 4;
  const int page_mask = p.page_size - 1;
  uint32_t koff[4], voff[4];
  auto set_offsets = [&](int maxr) {
    const int c16 = lane & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int R = 4 * i + g4;
      koff[i] = (uint32_t)(min(R, maxr) * (int)a.k_slot_b + ((c16 ^ R) << 4));
      voff[i] = (uint32_t)(min(R, maxr) * (int)a.v_slot_b + ((c16 ^ ((R & 7) | ((wave & 1) << 3))) << 4));
    }
  };
  set_offsets(15);
  bool tail = false;                                       // offsets clamped for the sequence's last, partial group
  const uint32_t lds0 = lds_addr(smem);
  auto group_of = [&](int tile) { return min(tile * 4 + wave, last_group); };     // stays inside the sequence's pages
  auto entry_off = [&](int tile) { return ((group_of(tile) << 4) >> a.page_shift) << 2; };
  auto issue_dma = [&](int tile, int page, int stage) {
    const int key0 = group_of(tile) << 4;
    const int maxr = seq_len - 1 - key0;
    if (maxr < 15 && !tail) { set_offsets(max(maxr, 0)); tail = true; }    // (only ever the last group, and every later fetch repeats it)
    const uint32_t slot0 = (uint32_t)(key0 & page_mask);
    const uint64_t kb = (uint64_t)kbase + (uint64_t)(uint32_t)page * a.k_page_b + (uint64_t)slot0 * a.k_slot_b;
    const uint64_t vb = (uint64_t)vbase + (uint64_t)(uint32_t)page * a.v_page_b + (uint64_t)slot0 * a.v_slot_b;
    const uint32_t dst = lds0 + (uint32_t)(stage * kFStageB + wave * (16 * kFRowB));
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16_s(koff[i], kb, dst + i * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16_s(voff[i], vb, dst + kFTileB + i * 1024);
  };

  // ---- per-lane LDS read offsets inside a stage (swizzle folded in) --------------------------------------------
  // K read n = 4 kt + kp: row 16 kt + r16, logical chunk 4 kp + g4  ->  k_rd[kp] + 4096 kt
  int k_rd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) k_rd[j] = r16 * kFRowB + (((4 * j + g4) ^ r16) << 4);
  // V read i = 16 c + db: lane pair r8 of the quarter wave addresses key row 16 (r8 >> 2) + 4 g4 + (r8 & 3) of the 32 keys of
  // k-step c, logical chunk db, its half r16 & 1  ->  v_rd[db] + 8192 c
  const int r8 = r16 >> 1, vrow = 16 * (r8 >> 2) + 4 * g4 + (r8 & 3);
  int v_rd[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v_rd[j] = kFTileB + vrow * kFRowB + ((j ^ ((vrow & 7) | ((vrow & 16) >> 1))) << 4) + 8 * (r16 & 1);

  float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};

  int pg = 0;                                              // the next tile's page (SGPR)
  if (tile_lo < tile_hi) {
    d_sload_start(pg, bt, entry_off(tile_lo));
    d_sload_land(pg);
    issue_dma(tile_lo, pg, 0);
    if (tile_lo + 1 < tile_hi) { d_sload_start(pg, bt, entry_off(tile_lo + 1)); d_sload_land(pg); }
  }

  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int stage = (tile - tile_lo) & 1;
    glds_wait_all();                                       // this wave's share of the tile has landed ...
    __syncthreads();                                       // ... and everyone's; the other stage's readers are done
    const bool has_next = tile + 1 < tile_hi;
    const bool has_next2 = tile + 2 < tile_hi;
    int pg2 = 0;
    if (has_next) {
      issue_dma(tile + 1, pg, stage ^ 1);
      if (has_next2) d_sload_start(pg2, bt, entry_off(tile + 2));
    }
    const char* st = smem + stage * kFStageB;
    const int key_base = tile * kDTile;

    if (wave_has_rows && key_base < wave_keys && (!SW || key_base + kDTile > wave_first_key)) {
      // ---- S^T = K . Q'^T: read n holds fragments m = 2 n and 2 n + 1 (kt = m >> 3, ks = m & 7), each feeds both row blocks;
      //      a ring of KW reads ahead of the converts, which run a fragment and a half ahead of the matrix instructions ----
      df32x4_t s[2][4];
      constexpr int KW = 4;
      du32x4_t rk[KW];
      uint32_t kx[3][4];                                   // fragments m, m + 1, m + 2 in the making
      auto k_raw = [&](int n) { return *(const du32x4_t*)(st + k_rd[n & 3] + 4096 * (n >> 2)); };
#pragma unroll
      for (int n = 0; n < KW; ++n) rk[n] = k_raw(n);
      wid::half(kx[0][0], kx[0][1], rk[0][0]);
      wid::half(kx[0][2], kx[0][3], rk[0][1]);
      wid::half(kx[1][0], kx[1][1], rk[0][2]);
      asm volatile("s_nop 1" ::: "memory");                // VALU-written K -> matrix instruction
      d_for<32>([&](auto M) __attribute__((always_inline)) {
        constexpr int m = decltype(M)::value, n = m >> 1, kt = m >> 3, ks = m & 7, b = m % 3;
        const du32x4_t kf = {kx[b][0], kx[b][1], kx[b][2], kx[b][3]};
        if constexpr (ks == 0) ops::template qk_zero<kDAccQ + 4 * ks>(s[0][kt], kf);
        else ops::template qk_acc<kDAccQ + 4 * ks>(s[0][kt], kf);
        if constexpr (m + 1 < 32) wid::half(kx[(m + 1) % 3][2], kx[(m + 1) % 3][3], rk[((m + 1) >> 1) % KW][2 * ((m + 1) & 1) + 1]);
        if constexpr (ks == 0) ops::template qk_zero<kDAccQ + 32 + 4 * ks>(s[1][kt], kf);
        else ops::template qk_acc<kDAccQ + 32 + 4 * ks>(s[1][kt], kf);
        if constexpr (m + 2 < 32) wid::half(kx[(m + 2) % 3][0], kx[(m + 2) % 3][1], rk[((m + 2) >> 1) % KW][2 * ((m + 2) & 1)]);
        if constexpr ((m & 1) == 0 && n + KW < 16) rk[n % KW] = k_raw(n + KW);     // (read n's last word went into fragment 2 n + 1 above)
      });
      // the matrix pipe's results are readable (the compiler does not know these statements are matrix instructions)
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3"
                   : "+v"(s[0][0]), "+v"(s[0][1]), "+v"(s[0][2]), "+v"(s[0][3]), "+v"(s[1][0]), "+v"(s[1][1]), "+v"(s[1][2]), "+v"(s[1][3]));

      // ---- softmax (log2 domain): register r of key block kt <-> key key_base + 16 kt + 4 g4 + r ----
      bool need_mask = (key_base + kDTile - 1 > ctx_len + w_tok_lo) || (key_base + kDTile > seq_len);
      if (SW) need_mask = need_mask || key_base < ctx_len + w_tok_hi - sw + 1;
      float m_use[2], alpha[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        if (need_mask) {
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = key_base + 16 * kt + 4 * g4 + r;
              const bool ok = key <= lim[rb] && (!SW || key >= lo_key[rb]);
              s[rb][kt][r] = ok ? s[rb][kt][r] : -INFINITY;
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[rb][kt][r]);
        mx = fmaxf(mx, lane_xor16(mx));                    // the other three quarter waves hold the row's other keys
        mx = fmaxf(mx, lane_xor32(mx));
        float m_new = fmaxf(m_run[rb], mx);
        if (m_run[rb] > -INFINITY && mx <= m_run[rb] + kDDefer) m_new = m_run[rb];
        m_use[rb] = m_new > -INFINITY ? m_new : 0.0f;      // a row without a visible key so far: P = 2^(-inf - 0) = 0
        // (a row's first visible keys: O and l are still 0, nothing to rescale)
        alpha[rb] = (m_new == m_run[rb] || !(m_run[rb] > -INFINITY)) ? 1.0f : __builtin_amdgcn_exp2f(m_run[rb] - m_use[rb]);
        m_run[rb] = m_new;
      }
      // P of the first 32 keys (k-step 0 of P.V), both row blocks
      du32x4_t pf[2][2];
      float psum[2] = {0.0f, 0.0f};
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { e[j] = __builtin_amdgcn_exp2f(s[rb][j >> 2][j & 3] - m_use[rb]); psum[rb] += e[j]; }
        pf[rb][0] = du32x4_t{ops::pack2(e[0], e[1]), ops::pack2(e[2], e[3]), ops::pack2(e[4], e[5]), ops::pack2(e[6], e[7])};
      }
      // ---- O^T = alpha O^T, only when some row's reference moved ----
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        if (!__all(alpha[rb] == 1.0f)) {
          asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");      // the previous tile's last P.V results are in their registers
          const float al = alpha[rb];
          if (rb == 0) d_for<64>([&](auto I) __attribute__((always_inline)) { constexpr int i = kDAccO + decltype(I)::value; d_acc_write<i>(f32_to_bits(d_acc_read<i>() * al)); });
          else d_for<64>([&](auto I) __attribute__((always_inline)) { constexpr int i = kDAccO + 64 + decltype(I)::value; d_acc_write<i>(f32_to_bits(d_acc_read<i>() * al)); });
          asm volatile("s_nop 3" ::: "memory");
        }
        l_run[rb] *= alpha[rb];
      }
      // ---- O^T += V^T . P^T: fragment i = 16 c + db is ONE transposed read, feeds both row blocks; a ring of VW reads ----
      constexpr int VW = 8;
      du32x2_t rv[VW];
      uint32_t vx[3][4];
      auto v_raw = [&](int i) {
        const di32x2_t v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) di32x2_t*)(st + v_rd[i & 15] + 8192 * (i >> 4)));
        return __builtin_bit_cast(du32x2_t, v);
      };
#pragma unroll
      for (int i = 0; i < VW; ++i) rv[i] = v_raw(i);
      wid::half(vx[0][0], vx[0][1], rv[0][0]);
      wid::half(vx[0][2], vx[0][3], rv[0][1]);
      wid::half(vx[1][0], vx[1][1], rv[1][0]);
      float e1[2][8];
      asm volatile("s_nop 1" ::: "memory");                // VALU-written P and V -> matrix instruction
      d_for<32>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value, c = i >> 4, db = i & 15;
        if constexpr (i == 16) {                             // P of the second 32 keys: its exponentials sit in the k-step 0 stream
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) psum[rb] += e1[rb][j];
            pf[rb][1] = du32x4_t{ops::pack2(e1[rb][0], e1[rb][1]), ops::pack2(e1[rb][2], e1[rb][3]), ops::pack2(e1[rb][4], e1[rb][5]), ops::pack2(e1[rb][6], e1[rb][7])};
          }
          asm volatile("s_nop 1" ::: "memory");
        }
        const du32x4_t vf = {vx[i % 3][0], vx[i % 3][1], vx[i % 3][2], vx[i % 3][3]};
        ops::template pv<kDAccO + 4 * db>(vf, pf[0][c]);
        if constexpr (i + 1 < 32) wid::half(vx[(i + 1) % 3][2], vx[(i + 1) % 3][3], rv[(i + 1) % VW][1]);
        ops::template pv<kDAccO + 64 + 4 * db>(vf, pf[1][c]);
        if constexpr (i + 2 < 32) wid::half(vx[(i + 2) % 3][0], vx[(i + 2) % 3][1], rv[(i + 2) % VW][0]);
        if constexpr (i + VW < 32) rv[i % VW] = v_raw(i + VW);
        if constexpr (i < 16) {
          constexpr int rb = i >> 3, j = i & 7;
          e1[rb][j] = d_exp2(s[rb][2 + (j >> 2)][j & 3] - m_use[rb]);
        }
      });
      l_run[0] += psum[0];
      l_run[1] += psum[1];
    }
    if (has_next2) { d_sload_land(pg2); pg = pg2; }
  }

  // ---- epilogue: lane (r16, g4) register r of block db of row block rb <-> row 16 rb + r16, column 16 db + 4 g4 + r ----
  float inv[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    float l = l_run[rb], m = m_run[rb];
    l += lane_xor16(l);
    l += lane_xor32(l);
    // attention sink: the row's (m, l) is final here
    const float sink_w = (p.sinks && row_ok[rb]) ? fold_sink<true>(m, l, p.sinks[hq[rb]]) : 1.0f;
    float* const lse_base = KS ? p.lse + (int64_t)ksplit * a.lse_split_stride : p.lse;
    if (lse_base && row_ok[rb] && g4 == 0)
      lse_base[(int64_t)(q_start + tok_local[rb]) * p.lse_stride_token + hq[rb]] = l > 0.0f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : -INFINITY;
    inv[rb] = (row_ok[rb] && l > 0.0f) ? v_sc * sink_w / l : 0.0f;      // (V was summed unscaled)
  }
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");   // the last P.V results are in their registers
  __syncthreads();                                              // every wave is done with the stages: O leaves through them
  // whole rows, 16 bytes per lane, nontemporal: parked per wave as 32 rows of 512 + 16 bytes
  char* ost = smem + wave * (32 * kDORS);
  d_for<2>([&](auto RB) __attribute__((always_inline)) {
    d_for<16>([&](auto DB) __attribute__((always_inline)) {
      constexpr int rb = decltype(RB)::value, db = decltype(DB)::value, o = kDAccO + 64 * rb + 4 * db;
      const float iv = inv[rb];
      const du32x2_t w = {ops::pack2(d_acc_read<o>() * iv, d_acc_read<o + 1>() * iv), ops::pack2(d_acc_read<o + 2>() * iv, d_acc_read<o + 3>() * iv)};
      *(du32x2_t*)(ost + (16 * rb + r16) * kDORS + (16 * db + 4 * g4) * 2) = w;
    });
  });
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int orow = lane >> 5, och = lane & 31;
  uint16_t* const out_base = KS ? (uint16_t*)p.out + (int64_t)ksplit * a.out_split_stride : (uint16_t*)p.out;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int r = 2 * j + orow;
    const int m = wave * 32 + r;
    const int tok = tok0 + m / G;
    const du32x4_t v = *(const du32x4_t*)(ost + r * kDORS + och * 16);
    if (m < BQ * G && tok < q_len)
      __builtin_nontemporal_store(v, (du32x4_t*)(out_base + (int64_t)(q_start + tok) * p.out_stride_token +
                                                 (int64_t)(head * G + m % G) * p.out_stride_head + och * 8));
  }
}

// ---------------------------------------------------------------------------------------------
// host side (the conditions: prefill_d256_applicable(), prefill_d256.hip)
// ---------------------------------------------------------------------------------------------
template <typename T, typename KVT, bool SW, bool KS>
static int launch_d256_fp8_t(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  D256Args a;
  a.p = p;
  a.group = p.num_q_heads / p.num_kv_heads;
  a.block_q = kDRows / a.group;
  a.page_shift = __builtin_ctz((unsigned)p.page_size);
  a.k_page_b = (uint32_t)p.k_stride_page; a.k_slot_b = (uint32_t)p.k_stride_slot;      // one byte an element
  a.v_page_b = (uint32_t)p.v_stride_page; a.v_slot_b = (uint32_t)p.v_stride_slot;
  a.key_splits = KS ? ks->splits : 1;
  a.out_split_stride = KS ? ks->out_split_stride : 0;
  a.lse_split_stride = KS ? ks->lse_split_stride : 0;
  const int qblocks = p.num_tokens / a.block_q + p.num_seqs;   // static upper bound, as for the other Q-block kernels
  static std::atomic<uint64_t> lds_opt_in{0};
  const int rc0 = ensure_dynamic_lds((const void*)prefill_d256_fp8_kernel<T, KVT, SW, KS>, kFLds, lds_opt_in, "hipFuncSetAttribute(prefill_d256_fp8)");
  if (rc0 != MI355_OK) return rc0;
  hipLaunchKernelGGL((prefill_d256_fp8_kernel<T, KVT, SW, KS>), dim3(qblocks * p.num_kv_heads, a.key_splits), dim3(256), kFLds, stream, a);
  const int rc = check_hip(hipGetLastError(), "prefill_d256_fp8_kernel launch");
  if (rc == MI355_OK) set_kernel_name(SW ? "prefill_mfma_fp8_d256_sw" : "prefill_mfma_fp8_d256");
  return rc;
}

template <typename T, typename KVT>
static int launch_d256_fp8_sw(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  if (ks) return p.sliding_window > 0 ? launch_d256_fp8_t<T, KVT, true, true>(p, stream, ks) : launch_d256_fp8_t<T, KVT, false, true>(p, stream, ks);
  return p.sliding_window > 0 ? launch_d256_fp8_t<T, KVT, true, false>(p, stream, ks) : launch_d256_fp8_t<T, KVT, false, false>(p, stream, ks);
}

int launch_prefill_d256_fp8(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  const bool fp8 = p.kv_dtype == MI355_FP8_E4M3 || p.kv_dtype == MI355_FP8_E5M2;
  if (!fp8 || !prefill_supported(p) || !prefill_d256_applicable(p) || (ks && (ks->splits < 2 || !p.lse || p.sinks))) {
    set_error("prefill_d256_fp8_kernel does not support this configuration");
    return MI355_ERR_UNSUPPORTED;
  }
  const bool bf = p.q_dtype == MI355_BF16;
  if (p.kv_dtype == MI355_FP8_E4M3) return bf ? launch_d256_fp8_sw<bf16_t, e4m3_t>(p, stream, ks) : launch_d256_fp8_sw<f16_t, e4m3_t>(p, stream, ks);
  return bf ? launch_d256_fp8_sw<bf16_t, e5m2_t>(p, stream, ks) : launch_d256_fp8_sw<f16_t, e5m2_t>(p, stream, ks);
}

}  // namespace mi355
