// prefill_d256_kernel: causal prefill attention at head size 256 (bf16 / f16, 16-bit cache, with or without a sliding
// window). Four waves, one per SIMD, 32 query rows each; K/V tiles of 64 keys by LDS-DMA; O and Q in accumulator registers
// that only the asm statements below name.
//
// Same semantics as prefill_mfma_kernel<T, T, 256, *> (prefill_mfma.hip), which served this head size alone before:
// a Q block is 128 rows (token, head-in-group) of one KV head, attended causally over the paged cache.
//
// Registers (per lane; the wave owns the whole 512-entry file, one workgroup per CU):
//   a[0..127]    O^T[rb][db]  : 64 rb + 4 db .. + 3   (rb = 16-row block 0 / 1 of the wave, db = 16-column block of the head)
//   a[128..191]  Q'[rb][ks]   : 128 + 32 rb + 4 ks .. + 3   (the query rows times scale * log2(e), ks = 32-wide k-step)
//   VGPRs        S^T (2 x 4 x 4 f32), P (2 x 2 x 4 packed words), the K / V fragment rings, softmax state, LDS-DMA offsets.
// Both contractions run on v_mfma_f32_16x16x32_{bf16,f16} in the "swapped" orientation of the other kernels here:
//   S^T = K . Q'^T   (A = 16 keys x 32 dims from LDS, B = Q' from a[..]):  4 key blocks x 8 k-steps x 2 row blocks = 64 / tile
//   O^T += V^T . P^T (A = 16 dims x 32 keys by ds_read_b64_tr_b16, B = P):  16 column blocks x 2 k-steps x 2 row blocks = 64 / tile
// so lane (q = lane & 15, g = lane >> 4) owns query rows q and 16 + q of the wave: its S registers are keys 16 kt + 4 g + r of
// those rows, the row maximum is 15 v_max + two lane exchanges, and the packed S registers ARE the B operand of P.V
// (k-slot e of k-step c = key 32 c + 16 (e >> 2) + 4 g + (e & 3)); the transposed V read is addressed to deliver that order.
// Every K and V fragment is read from LDS once per tile and feeds both row blocks: 64 KiB of LDS reads per wave and tile.
//
// LDS (128 KiB of the CU's 160): two stages of [K tile 32 KiB | V tile 32 KiB], rows of 512 bytes = 32 chunks of 16 bytes,
// unpadded (an LDS-DMA instruction writes 1 KiB = two key rows contiguously), bank conflicts avoided by an XOR on the chunk
// index, applied on the per-lane SOURCE offset and again on the read address:
//   K (ds_read_b128, sixteen rows x one chunk per quarter wave):            chunk ^= row & 15
//   V (ds_read_b64_tr_b16, eight rows x two chunks per half wave):          chunk ^= 2 (row & 7)
// Wave w stages key rows 16 w .. 16 w + 15 of every tile: ONE block-table entry per wave and tile (pages hold >= 16 keys),
// read through the scalar cache a tile ahead, a scalar page base and sixteen constant per-lane offsets - no staging
// registers, no VALU copy. Rows past the sequence re-read its last row (finite data under P = 0).
//
// Pipeline: tile t + 1's LDS-DMA is issued before tile t's compute and retired (vmcnt) before the ONE barrier per tile
// that publishes it. The exponentials of a tile's second 32 keys are dealt one per V fragment into the first 32 keys' P.V
// matrix instructions.
//
// Softmax: online, base 2, a true running maximum per row, moved only when a tile's maximum exceeds it by more than 2^8
// (P <= 2^8: exact in f32 sums, far inside bf16 / f16; rescaling O is 128 trips through the accumulator registers).
// No fixed reference, so f16 needs no range check and no fix-up launch. Only tiles on the diagonal, the sequence's last
// partial tile and (SW) the window's edge tiles are masked.
//
// Key-split form (KS, library 0.13.0; grid.y = splits): workgroup (x, s) walks the s-th even share of its Q block's own tile
// range - from the window's first tile with SW - and writes normalised partial rows (query type) and their lse (f32) to the
// workspace buffers of split s; merge_key_splits_kernel (prefill_mfma.hip) folds them and adds the sink, once. Nothing else
// changes: the prefetch starts at the share's first tile, stage parity counts from it, masks and the tail clamp are functions
// of absolute key positions; a share without a tile, or without a visible key for a row, leaves that row at out 0 / lse -inf.
// The one-pass instantiations (KS = false) keep their code.
#include <cstdlib>

#include "prefill_d256.h"

namespace mi355 {

constexpr int kDRowB = 512;                 // bytes per key row (256 x 2)
constexpr int kDTileB = kDTile * kDRowB;    // 32 KiB: one K or V tile
constexpr int kDStageB = 2 * kDTileB;       // K tile then V tile
constexpr int kDLds = 2 * kDStageB;         // two stages
static_assert(4 * 32 * kDORS <= kDLds && kDLds <= 160 * 1024, "prefill_d256_kernel: LDS map");

template <typename T, bool SW, bool KS>
__global__ __launch_bounds__(256, 1) void prefill_d256_kernel(const D256Args a) {
  using ops = d256_ops<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  asm volatile("" ::: "a255");                 // the kernel owns all 256 accumulator registers

  const mi355_attn_params& p = a.p;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = a.group, BQ = a.block_q;

  // 1-D grid, KV head fastest (one KV head per XCD's L2 with Hk = 8), heaviest Q blocks first (prefill_mfma_kernel)
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

  // ---- Q' = Q * scale * log2(e) into a[128 ..]: lane (r16, g4) holds Q'[row][32 ks + 8 g4 .. + 7] --------------
  const float scale2 = p.scale * kDLog2e;
  // (all sixteen loads in flight together: a row outside the Q block reads the sequence's last query token instead - always
  // a valid address - and is scaled by 0)
  {
    du32x4_t qv[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const uint16_t* qp = (const uint16_t*)p.q + (int64_t)(q_start + min(tok_local[rb], q_len - 1)) * p.q_stride_token + (int64_t)hq[rb] * p.q_stride_head + 8 * g4;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) qv[rb][ks] = *(const du32x4_t*)(qp + 32 * ks);
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

  // ---- LDS-DMA: wave w stages key rows 16 w .. 16 w + 15 of a tile, two rows per instruction ------------------
  // instruction i: LDS row R = 2 i + (lane >> 5), chunk position lane & 31 holds logical chunk position ^ f(R)
  const int32_t* bt = p.block_table + (int64_t)seq * p.block_table_stride;
  const char* kbase = (const char*)p.k_cache + (int64_t)head * p.k_stride_head * 2;
  const char* vbase = (const char*)p.v_cache + (int64_t)head * p.v_stride_head * 2;
  const int last_group = (max(seq_len, 1) - 1) >> 4;
  const int page_mask = p.page_size - 1;
  uint32_t koff[8], voff[8];
  auto set_offsets = [&](int maxr) {
    const int h = lane >> 5, c32 = lane & 31;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int R = 2 * i + h;
      koff[i] = (uint32_t)(min(R, maxr) * (int)a.k_slot_b + ((c32 ^ R) << 4));
      voff[i] = (uint32_t)(min(R, maxr) * (int)a.v_slot_b + ((c32 ^ (2 * (R & 7))) << 4));
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
    const uint32_t dst = lds0 + (uint32_t)(stage * kDStageB + wave * (16 * kDRowB));
#pragma unroll
    for (int i = 0; i < 8; ++i) glds16_s(koff[i], kb, dst + i * 1024);
#pragma unroll
    for (int i = 0; i < 8; ++i) glds16_s(voff[i], vb, dst + kDTileB + i * 1024);
  };

  // ---- per-lane LDS read offsets inside a stage (swizzle folded in) --------------------------------------------
  // K fragment (kt, ks): row 16 kt + r16, logical chunk 4 ks + g4  ->  k_rd[ks & 3] + 256 (ks >> 2) + 8192 kt
  int k_rd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) k_rd[j] = r16 * kDRowB + (((4 * j + g4) ^ r16) << 4);
  // V fragment (db, c): two transposed reads of the 4-key x 16-column blocks at keys 32 c + 4 g4 and + 16; lane 4 q4 + pp of
  // a quarter wave addresses key row q4 of the block, columns 4 pp .. + 3  ->  v_rd[db & 7] + 256 (db >> 3) + 8192 j + 16384 c
  const int q4 = r16 >> 2, pp = r16 & 3, vrow = 4 * g4 + q4;
  int v_rd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v_rd[j] = kDTileB + vrow * kDRowB + (((2 * j + (pp >> 1)) ^ (2 * (vrow & 7))) << 4) + 8 * (pp & 1);

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
    const char* st = smem + stage * kDStageB;
    const int key_base = tile * kDTile;

    if (wave_has_rows && key_base < wave_keys && (!SW || key_base + kDTile > wave_first_key)) {
      // ---- S^T = K . Q'^T: fragment m = 8 kt + ks feeds both row blocks; a ring of KW fragments ahead of the matrix pipe ----
      df32x4_t s[2][4];
      constexpr int KW = 8;
      du32x4_t kf[KW];
      auto k_frag = [&](int m) { return *(const du32x4_t*)(st + k_rd[m & 3] + 256 * ((m >> 2) & 1) + 8192 * (m >> 3)); };
#pragma unroll
      for (int m = 0; m < KW; ++m) kf[m] = k_frag(m);
      d_for<32>([&](auto M) __attribute__((always_inline)) {
        constexpr int m = decltype(M)::value, kt = m >> 3, ks = m & 7;
        if constexpr (ks == 0) {
          ops::template qk_zero<kDAccQ + 4 * ks>(s[0][kt], kf[m % KW]);
          ops::template qk_zero<kDAccQ + 32 + 4 * ks>(s[1][kt], kf[m % KW]);
        } else {
          ops::template qk_acc<kDAccQ + 4 * ks>(s[0][kt], kf[m % KW]);
          ops::template qk_acc<kDAccQ + 32 + 4 * ks>(s[1][kt], kf[m % KW]);
        }
        if constexpr (m + KW < 32) kf[m % KW] = k_frag(m + KW);
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
      // ---- O^T += V^T . P^T: fragment i = 16 c + db feeds both row blocks; a ring of VW fragments ----
      constexpr int VW = 8;
      du32x4_t vt[VW];
      auto v_frag = [&](int i) {
        const char* va = st + v_rd[i & 7] + 256 * ((i >> 3) & 1) + 16384 * (i >> 4);
        const ds16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ds16x4_t*)(va));
        const ds16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ds16x4_t*)(va + 8192));
        const du32x2_t w0 = __builtin_bit_cast(du32x2_t, v0), w1 = __builtin_bit_cast(du32x2_t, v1);
        return du32x4_t{w0[0], w0[1], w1[0], w1[1]};
      };
#pragma unroll
      for (int i = 0; i < VW; ++i) vt[i] = v_frag(i);
      float e1[2][8];
      asm volatile("s_nop 1" ::: "memory");                // VALU-written P -> matrix instruction
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
        ops::template pv<kDAccO + 4 * db>(vt[i % VW], pf[0][c]);
        ops::template pv<kDAccO + 64 + 4 * db>(vt[i % VW], pf[1][c]);
        if constexpr (i + VW < 32) vt[i % VW] = v_frag(i + VW);
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
    inv[rb] = (row_ok[rb] && l > 0.0f) ? sink_w / l : 0.0f;
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
// host side
// ---------------------------------------------------------------------------------------------
// Beyond prefill_supported(): exactly head size 256, a 16-bit cache of the query's type or an fp8 cache (library 0.10.0:
// prefill_d256_fp8.hip), causal, no soft-cap / ALiBi, no fused cache write, output rows the 16-byte stores can address.
bool prefill_d256_applicable(const mi355_attn_params& p) {
  const bool fp8 = p.kv_dtype == MI355_FP8_E4M3 || p.kv_dtype == MI355_FP8_E5M2;
  if (p.head_size != 256 || (p.kv_dtype != p.q_dtype && !fp8)) return false;
  if (p.softcap > 0.0f || p.alibi_slopes || p.non_causal || p.write_new_kv || p.k_new || p.v_new) return false;
  if (((uintptr_t)p.out & 15) != 0 || p.out_stride_token % 8 != 0 || p.out_stride_head % 8 != 0) return false;
  const int64_t eb = fp8 ? 1 : 2;                                                                  // bytes per cache element
  if (p.k_stride_page * eb >= (1LL << 32) || p.v_stride_page * eb >= (1LL << 32)) return false;    // byte strides in 32 bits
  if (fp8) {                                                                                       // 16-byte LDS-DMA pieces of fp8 rows
    const int64_t strides[] = {p.k_stride_page, p.k_stride_slot, p.k_stride_head, p.v_stride_page, p.v_stride_slot, p.v_stride_head};
    for (int64_t s : strides) if (s % 16 != 0) return false;
  }
  return true;
}

template <typename T, bool SW, bool KS>
static int launch_d256_t(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  D256Args a;
  a.p = p;
  a.group = p.num_q_heads / p.num_kv_heads;
  a.block_q = kDRows / a.group;
  a.page_shift = __builtin_ctz((unsigned)p.page_size);
  a.k_page_b = (uint32_t)(p.k_stride_page * 2); a.k_slot_b = (uint32_t)(p.k_stride_slot * 2);
  a.v_page_b = (uint32_t)(p.v_stride_page * 2); a.v_slot_b = (uint32_t)(p.v_stride_slot * 2);
  a.key_splits = KS ? ks->splits : 1;
  a.out_split_stride = KS ? ks->out_split_stride : 0;
  a.lse_split_stride = KS ? ks->lse_split_stride : 0;
  const int qblocks = p.num_tokens / a.block_q + p.num_seqs;   // static upper bound, as for the other Q-block kernels
  static std::atomic<uint64_t> lds_opt_in{0};
  const int rc0 = ensure_dynamic_lds((const void*)prefill_d256_kernel<T, SW, KS>, kDLds, lds_opt_in, "hipFuncSetAttribute(prefill_d256)");
  if (rc0 != MI355_OK) return rc0;
  hipLaunchKernelGGL((prefill_d256_kernel<T, SW, KS>), dim3(qblocks * p.num_kv_heads, a.key_splits), dim3(256), kDLds, stream, a);
  const int rc = check_hip(hipGetLastError(), "prefill_d256_kernel launch");
  if (rc == MI355_OK) set_kernel_name(SW ? "prefill_mfma_d256_sw" : "prefill_mfma_d256");
  return rc;
}

template <typename T>
static int launch_d256_sw(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  if (ks) return p.sliding_window > 0 ? launch_d256_t<T, true, true>(p, stream, ks) : launch_d256_t<T, false, true>(p, stream, ks);
  return p.sliding_window > 0 ? launch_d256_t<T, true, false>(p, stream, ks) : launch_d256_t<T, false, false>(p, stream, ks);
}

// ks: the key-split launch (launch_prefill_ws: p.out / p.lse are the workspace's partial buffers and never null, p.sinks is
// null - the merge behind this launch folds the sink in, once - and the name gets its _ksplit suffix there)
int launch_prefill_d256(const mi355_attn_params& p, hipStream_t stream, const KeySplitCtx* ks) {
  if (!prefill_supported(p) || !prefill_d256_applicable(p) || (ks && (ks->splits < 2 || !p.lse || p.sinks))) {
    set_error("prefill_d256_kernel does not support this configuration");
    return MI355_ERR_UNSUPPORTED;
  }
  if (p.kv_dtype != p.q_dtype) return launch_prefill_d256_fp8(p, stream, ks);
  return p.q_dtype == MI355_BF16 ? launch_d256_sw<bf16_t>(p, stream, ks) : launch_d256_sw<f16_t>(p, stream, ks);
}

}  // namespace mi355
