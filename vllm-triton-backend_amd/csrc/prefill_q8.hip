// prefill_q8_kernel: causal prefill attention at head size 128 with fp8 (e4m3) QUERIES over an fp8 cache (e4m3 / e5m2), with or
// without a sliding window, bf16 output (library 0.11.0). Nothing is widened: Q, K, V and P all enter
// v_mfma_f32_16x16x128_f8f6f4 as bytes - twice the bf16 rate per FLOP, and one instruction contracts the whole head dimension.
//
// Work split: a workgroup of four waves serves one Q block - 128 rows (token, head of the group) of one KV head of one
// sequence - each wave 32 rows as two 16-row blocks; two workgroups share a CU (2 x 64 KiB of LDS, <= 256 registers a lane),
// so a SIMD holds two waves and one's exponentials run under the other's matrix instructions.
//
// Operand layout of the 16x16x128 instruction: lane (i = lane & 15, g = lane >> 4) holds 32 bytes of row i of A (column i of
// B); which 32 of the 128 contraction slots those are is the same function of (g, byte) for A and for B, so a contraction
// only needs both operands to put the SAME thing in byte b of lane group g. The result is the usual 16x16 one: lane (i, g)
// holds column i, rows 4 g .. 4 g + 3.
//
//   S^T = K . Q^T   A = K: byte b of group g is head dim 32 g + b of key row 16 kt + i - two plain 16-byte LDS reads;
//                   B = Q: the same 32 bytes of query row i, read once from global memory and kept (16 registers a wave).
//                   Lane (i, g) then holds, for query i, keys 16 kt + 4 g + r (r = 0 .. 3) of each of the tile's 8 key blocks.
//   O^T += V^T . P^T  B = P: byte 4 kt + r of group g is the lane's OWN score of key 16 kt + 4 g + r, packed where it stands by
//                   v_cvt_pk_fp8_f32 - P never crosses lanes; A = V^T must then hold V[key 16 kt + 4 g + r][dim 16 db + i] in
//                   byte 4 kt + r: ds_read_b64_tr_b8 (an [8][16] byte transpose inside a quarter wave, tools/probes/
//                   ds_read_tr8.hip) with lane pair r8 of quarter g addressing key row 32 c + 16 (r8 >> 2) + 4 g + (r8 & 3)
//                   delivers bytes 8 c .. 8 c + 7; four reads make an operand.
//   l += 1 . P^T    the row sums come from the ROUNDED P on the matrix pipe (A = a tile of ones), so numerator and denominator
//                   carry the same rounding.
//
// P enters both as TWO e4m3 terms: the weight rounded to e4m3 and its rounding residual (exact in fp32) rounded to e4m3 - each
// V operand feeds four instructions instead of two. One term alone (3 mantissa bits on the two or three weights that carry a
// row) measured 4e-2 .. 1e-1 of absolute error on the test inputs, whatever the scaling; two terms leave the bf16 rounding of
// the output as the largest error.
//
// P is exp2(c s - c m + 8): a true running maximum m, so P <= 2^8 - the upper e4m3 range (max 448), eight more binades above the
// subnormals than P <= 1 has. The factor 2^8 is in O and in l alike and leaves with O / l; lse subtracts it.
// c = scale * k_scale * log2(e) is one FMA per score in front of v_exp_f32; a negative c flips the sign bit of Q instead
// (exact in fp8) so that the maximum of the raw scores is the maximum of the scaled ones.
//
// LDS: two stages of [K tile | V tile], 128 keys x 128 bytes each (16 KiB), filled by LDS-DMA on a scalar page base: wave w
// stages key rows 32 w .. 32 w + 31 (inside one page: page size >= 32) with four instructions of eight rows for K and four for
// V, its block-table entry a tile ahead through the scalar cache. Rows of 128 bytes start on bank 0 or 32, so the 16-byte
// chunk index is XORed on the per-lane SOURCE offset and again on the read address:
//   K (ds_read_b128, a quarter wave reads 16 consecutive rows at one chunk):            chunk ^= (row >> 1) & 7
//   V (ds_read_b64_tr_b8, a half wave reads rows 32 c + {0 .. 7, 16 .. 23} or {8 .. 15, 24 .. 31}): chunk ^= ((row >> 1) & 3) | ((row >> 4) & 1) << 2
// Nothing outside the sequence reaches a sum: rows past it re-read its last row (valid data, never a stale 0x7f byte, and no
// page beyond the sequence's last), and a masked score is -inf by select, whose P is exactly 0.
#include <cstdlib>

#include "prefill_d256.h"      // D256Args, d_for, d_sload_start / d_sload_land, the vector types

namespace mi355 {

typedef __attribute__((ext_vector_type(8))) int qi32x8_t;
typedef __attribute__((ext_vector_type(2))) int qi32x2_t;
typedef __attribute__((ext_vector_type(2))) float qf32x2_t;

constexpr int kQRows = 128;                  // Q-block rows per workgroup
constexpr int kQTile = 128;                  // keys per tile = the contraction length of the second product
constexpr int kQRowB = 128;                  // bytes per key row
constexpr int kQTileB = kQTile * kQRowB;     // 16 KiB: one K or V tile
constexpr int kQStageB = 2 * kQTileB;        // K tile then V tile
constexpr int kQORS = 128 * 2 + 16;          // padded stride of the bf16 output rows parked in LDS (epilogue)
constexpr int kQLds = 2 * kQStageB;
constexpr float kQPShift = 8.0f;             // P = 2^8 exp(s - m)
static_assert(4 * 32 * kQORS <= kQLds && kQLds <= 64 * 1024, "prefill_q8_kernel: LDS map");

// D = A . B + C on fp8 operands; A in the cache's format, B (Q or P) always e4m3. Zero scale operands: the unscaled instruction.
template <bool E5>
__device__ __forceinline__ df32x4_t q8_mfma(const qi32x8_t& a, const qi32x8_t& b, const df32x4_t& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, E5 ? 1 : 0, 0, 0, 0, 0, 0);
}

template <bool E5, bool SW>
__global__ __launch_bounds__(256, 2) void prefill_q8_kernel(const D256Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const mi355_attn_params& p = a.p;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = a.group, BQ = a.block_q;

  // 1-D grid, KV head fastest, heaviest Q blocks first
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
  const int tile_lo = SW ? max(0, ctx_len + tok0 - sw + 1) / kQTile : 0;
  const int tile_hi = (n_keys_wg + kQTile - 1) / kQTile;

  // ---- scores are c * (q . k): |c| rides the exponent's FMA, its sign the queries ----
  const float c_signed = p.scale * kDLog2e * (p.k_scale ? p.k_scale[0] : 1.0f);
  const float c2 = fmaxf(fabsf(c_signed), 1.17549435e-38f);      // (never 0: a masked score's -inf times c stays -inf)
  const uint32_t q_flip = c_signed < 0.0f ? 0x80808080u : 0u;
  const float v_sc = p.v_scale ? p.v_scale[0] : 1.0f;

  // ---- Q: 32 bytes of each of the lane's two rows, head dims 32 g4 .. + 31; a row outside the Q block is zero ----
  qi32x8_t qf[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const char* qp = (const char*)p.q + (int64_t)(q_start + min(tok_local[rb], q_len - 1)) * p.q_stride_token + (int64_t)hq[rb] * p.q_stride_head + 32 * g4;
    const du32x4_t lo = *(const du32x4_t*)qp, hi = *(const du32x4_t*)(qp + 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qf[rb][j] = row_ok[rb] ? (int)(lo[j] ^ q_flip) : 0;
      qf[rb][4 + j] = row_ok[rb] ? (int)(hi[j] ^ q_flip) : 0;
    }
  }

  // ---- LDS-DMA: wave w stages key rows 32 w .. 32 w + 31 of a tile, eight rows per instruction ------------------
  // instruction i: LDS row R = 8 i + (lane >> 3) of the wave's 32, chunk position lane & 7 holds logical chunk position ^ f(R)
  // (f of the tile row 32 w + R is f of R for both swizzles)
  const int32_t* bt = p.block_table + (int64_t)seq * p.block_table_stride;
  const char* kbase = (const char*)p.k_cache + (int64_t)head * p.k_stride_head;
  const char* vbase = (const char*)p.v_cache + (int64_t)head * p.v_stride_head;
  const int last_group = (max(seq_len, 1) - 1) >> 5;
  const int page_mask = p.page_size - 1;
  const uint32_t lds0 = lds_addr(smem);
  auto group_of = [&](int tile) { return min(tile * 4 + wave, last_group); };     // stays inside the sequence's pages
  auto entry_off = [&](int tile) { return ((group_of(tile) << 5) >> a.page_shift) << 2; };
  auto issue_dma = [&](int tile, int page, int stage) {
    const int key0 = group_of(tile) << 5;
    const int maxr = seq_len - 1 - key0;                   // rows past the sequence's last re-read it
    const uint32_t slot0 = (uint32_t)(key0 & page_mask);
    const uint64_t kb = (uint64_t)kbase + (uint64_t)(uint32_t)page * a.k_page_b + (uint64_t)slot0 * a.k_slot_b;
    const uint64_t vb = (uint64_t)vbase + (uint64_t)(uint32_t)page * a.v_page_b + (uint64_t)slot0 * a.v_slot_b;
    const uint32_t dst = lds0 + (uint32_t)(stage * kQStageB + wave * (32 * kQRowB));
    const int c8 = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int R = 8 * i + (lane >> 3);
      glds16_s((uint32_t)(min(R, maxr) * (int)a.k_slot_b + ((c8 ^ ((R >> 1) & 7)) << 4)), kb, dst + i * 1024);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int R = 8 * i + (lane >> 3);
      glds16_s((uint32_t)(min(R, maxr) * (int)a.v_slot_b + ((c8 ^ (((R >> 1) & 3) | (((R >> 4) & 1) << 2))) << 4)), vb, dst + kQTileB + i * 1024);
    }
  };

  // ---- per-lane LDS read offsets inside a stage (swizzle folded in) --------------------------------------------
  // K block kt: row 16 kt + r16, logical chunks 2 g4 and 2 g4 + 1  ->  k_rd[j] + 2048 kt
  int k_rd[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) k_rd[j] = r16 * kQRowB + (((2 * g4 + j) ^ (r16 >> 1)) << 4);
  // V read (db, c): lane pair r8 of the quarter wave addresses key row 32 c + vrow, logical chunk db, its half r16 & 1
  //   ->  v_rd[db] + 4096 c
  const int r8 = r16 >> 1, vrow = 16 * (r8 >> 2) + 4 * g4 + (r8 & 3);
  int v_rd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v_rd[j] = kQTileB + vrow * kQRowB + ((j ^ (((vrow >> 1) & 3) | (((vrow >> 4) & 1) << 2))) << 4) + 8 * (r16 & 1);

  // O^T [128 dims x 32 queries] and the row sums: lane (r16, g4) register r of block db <-> query 16 rb + r16, dim 16 db + 4 g4 + r
  df32x4_t o[2][8], l_acc[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    l_acc[rb] = df32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int db = 0; db < 8; ++db) o[rb][db] = df32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
  }
  float m_run[2] = {-INFINITY, -INFINITY};                 // running maximum of the raw scores q . k
  const int one4 = E5 ? 0x3c3c3c3c : 0x38383838;           // 1.0 four times, in the cache's format
  const qi32x8_t ones = {one4, one4, one4, one4, one4, one4, one4, one4};

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
    const char* st = smem + stage * kQStageB;
    const int key_base = tile * kQTile;

    if (wave_has_rows && key_base < wave_keys && (!SW || key_base + kQTile > wave_first_key)) {
      // ---- S^T = K . Q^T: one instruction per key block and row block ----
      df32x4_t s[2][8];
      const df32x4_t zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        const du32x4_t k0 = *(const du32x4_t*)(st + k_rd[0] + 2048 * kt), k1 = *(const du32x4_t*)(st + k_rd[1] + 2048 * kt);
        const qi32x8_t kf = {(int)k0[0], (int)k0[1], (int)k0[2], (int)k0[3], (int)k1[0], (int)k1[1], (int)k1[2], (int)k1[3]};
        s[0][kt] = q8_mfma<E5>(kf, qf[0], zero);
        s[1][kt] = q8_mfma<E5>(kf, qf[1], zero);
      }

      // ---- softmax on the raw scores: register r of key block kt <-> key key_base + 16 kt + 4 g4 + r ----
      bool need_mask = (key_base + kQTile - 1 > ctx_len + w_tok_lo) || (key_base + kQTile > seq_len);
      if (SW) need_mask = need_mask || key_base < ctx_len + w_tok_hi - sw + 1;
      qi32x8_t pf[2], pl[2];                               // P = pf + pl: the rounded weights and their rounded residuals
      float alpha[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        if (need_mask) {
#pragma unroll
          for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = key_base + 16 * kt + 4 * g4 + r;
              const bool ok = key <= lim[rb] && (!SW || key >= lo_key[rb]);
              s[rb][kt][r] = ok ? s[rb][kt][r] : -INFINITY;
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
          mx = fmaxf(fmaxf(mx, s[rb][kt][0]), s[rb][kt][1]);     // v_max3_f32
          mx = fmaxf(fmaxf(mx, s[rb][kt][2]), s[rb][kt][3]);
        }
        mx = fmaxf(mx, lane_xor16(mx));                    // the other three quarter waves hold the row's other keys
        mx = fmaxf(mx, lane_xor32(mx));
        const float m_new = fmaxf(m_run[rb], mx);
        const float m_use = m_new > -INFINITY ? m_new : 0.0f;    // a row without a visible key so far: P = 2^(-inf) = 0
        // (a row's first visible keys: O and l are still 0, nothing to rescale)
        alpha[rb] = (m_new == m_run[rb] || !(m_run[rb] > -INFINITY)) ? 1.0f : __builtin_amdgcn_exp2f((m_run[rb] - m_use) * c2);
        m_run[rb] = m_new;
        const float off = kQPShift - m_use * c2;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
          const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[rb][kt][0], c2, off)), e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[rb][kt][1], c2, off));
          const float e2 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[rb][kt][2], c2, off)), e3 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[rb][kt][3], c2, off));
          const int hi = __builtin_amdgcn_cvt_pk_fp8_f32(e2, e3, __builtin_amdgcn_cvt_pk_fp8_f32(e0, e1, 0, false), true);
          const qf32x2_t h01 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), h23 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
          pf[rb][kt] = hi;
          pl[rb][kt] = __builtin_amdgcn_cvt_pk_fp8_f32(e2 - h23[0], e3 - h23[1], __builtin_amdgcn_cvt_pk_fp8_f32(e0 - h01[0], e1 - h01[1], 0, false), true);
        }
      }
      // ---- O^T = alpha O^T and l = alpha l, only when some row's maximum moved ----
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        if (!__all(alpha[rb] == 1.0f)) {
          l_acc[rb] *= alpha[rb];
#pragma unroll
          for (int db = 0; db < 8; ++db) o[rb][db] *= alpha[rb];
        }
      }
      // ---- O^T += V^T . P^T: four transposed reads make the operand of one dim block, which feeds both row blocks ----
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        qi32x8_t vf;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const qi32x2_t v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) qi32x2_t*)(st + v_rd[db] + 4096 * c));
          vf[2 * c] = v[0];
          vf[2 * c + 1] = v[1];
        }
        o[0][db] = q8_mfma<E5>(vf, pf[0], o[0][db]);
        o[1][db] = q8_mfma<E5>(vf, pf[1], o[1][db]);
        o[0][db] = q8_mfma<E5>(vf, pl[0], o[0][db]);
        o[1][db] = q8_mfma<E5>(vf, pl[1], o[1][db]);
      }
      l_acc[0] = q8_mfma<E5>(ones, pf[0], l_acc[0]);
      l_acc[1] = q8_mfma<E5>(ones, pf[1], l_acc[1]);
      l_acc[0] = q8_mfma<E5>(ones, pl[0], l_acc[0]);
      l_acc[1] = q8_mfma<E5>(ones, pl[1], l_acc[1]);
    }
    if (has_next2) { d_sload_land(pg2); pg = pg2; }
  }

  // ---- epilogue: (m, l) in the log2 domain of the scaled scores, l without P's factor ----
  float inv[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    float l = l_acc[rb][0] * 0.00390625f, m = m_run[rb] > -INFINITY ? m_run[rb] * c2 : -INFINITY;
    // attention sink: the row's (m, l) is final here
    const float sink_w = (p.sinks && row_ok[rb]) ? fold_sink<true>(m, l, p.sinks[hq[rb]]) : 1.0f;
    if (p.lse && row_ok[rb] && g4 == 0)
      p.lse[(int64_t)(q_start + tok_local[rb]) * p.lse_stride_token + hq[rb]] = l > 0.0f ? (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f : -INFINITY;
    inv[rb] = (row_ok[rb] && l > 0.0f) ? v_sc * sink_w * 0.00390625f / l : 0.0f;      // (V was summed unscaled, P times 2^8)
  }
  __syncthreads();                                              // every wave is done with the stages: O leaves through them
  // whole rows, 16 bytes per lane, nontemporal: parked per wave as 32 rows of 256 + 16 bytes
  char* ost = smem + wave * (32 * kQORS);
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const float iv = inv[rb];
      const du32x2_t w = {pack_bf16x2(o[rb][db][0] * iv, o[rb][db][1] * iv), pack_bf16x2(o[rb][db][2] * iv, o[rb][db][3] * iv)};
      *(du32x2_t*)(ost + (16 * rb + r16) * kQORS + (16 * db + 4 * g4) * 2) = w;
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int orow = lane >> 4, och = lane & 15;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = 4 * j + orow;
    const int m = wave * 32 + r;
    const int tok = tok0 + m / G;
    const du32x4_t v = *(const du32x4_t*)(ost + r * kQORS + och * 16);
    if (m < BQ * G && tok < q_len)
      __builtin_nontemporal_store(v, (du32x4_t*)((uint16_t*)p.out + (int64_t)(q_start + tok) * p.out_stride_token +
                                                 (int64_t)(head * G + m % G) * p.out_stride_head + och * 8));
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// What a call with fp8 queries must be (include/mi355_attn.h, q_dtype); the message names the first cause otherwise. Host
// arithmetic only.
bool prefill_q8_supported(const mi355_attn_params& p) {
  const bool kv8 = p.kv_dtype == MI355_FP8_E4M3 || p.kv_dtype == MI355_FP8_E5M2;
  const char* why = nullptr;
  if (p.q_dtype != MI355_FP8_E4M3) why = "e5m2 queries are not served (fp8 queries are e4m3)";
  else if (!kv8) why = "fp8 queries need an fp8 cache";
  else if (p.head_size != 128) why = "fp8 queries are served at head size 128 only";
  else if (p.softcap > 0.0f) why = "fp8 queries take no soft-cap";
  else if (p.alibi_slopes) why = "fp8 queries take no ALiBi slopes";
  else if (p.non_causal) why = "fp8 queries are causal only (non_causal)";
  else if (p.k_new || p.v_new) why = "fp8 queries read every key from the cache (k_new / v_new)";
  else if (p.write_new_kv) why = "fp8 queries carry no fused cache write (write_new_kv)";
  else if (p.kernel_select == MI355_SELECT_3D || p.kernel_select == MI355_SELECT_GENERIC) why = "fp8 queries run on the Q-block kernel only (MI355_SELECT_3D / MI355_SELECT_GENERIC)";
  else if (p.k_x != p.head_size || p.k_stride_d != 1 || p.v_stride_d != 1) why = "fp8 queries need the flash layout (not the legacy layout)";
  else if (p.num_segments > 1) why = "fp8 queries take no key-split plan (num_segments > 1)";
  else if (p.page_size < 32 || (p.page_size & (p.page_size - 1)) != 0) why = "fp8 queries need a page size that is a power of two >= 32";
  else if (p.num_q_heads / p.num_kv_heads > kQRows) why = "fp8 queries serve at most 128 query heads per KV head";
  else if (p.k_stride_page >= (1LL << 32) || p.v_stride_page >= (1LL << 32) || p.k_stride_slot >= (1LL << 24) || p.v_stride_slot >= (1LL << 24) ||
           p.k_stride_page <= 0 || p.v_stride_page <= 0 || p.k_stride_slot <= 0 || p.v_stride_slot <= 0) why = "fp8 queries: cache strides out of range";
  else {
    const int64_t strides[] = {p.k_stride_page, p.k_stride_slot, p.k_stride_head, p.v_stride_page, p.v_stride_slot, p.v_stride_head, p.q_stride_token, p.q_stride_head};
    for (int64_t s : strides) if (s % 16 != 0) why = "fp8 queries need every q / K / V stride to be a multiple of 16 elements";
    if ((((uintptr_t)p.q | (uintptr_t)p.k_cache | (uintptr_t)p.v_cache | (uintptr_t)p.out) & 15) != 0 || p.out_stride_token % 8 != 0 || p.out_stride_head % 8 != 0)
      why = "fp8 queries need 16-byte aligned q / out / caches and out strides that are multiples of 8 elements";
  }
  if (why) set_error("%s", why);
  return why == nullptr;
}

template <bool E5, bool SW>
static int launch_q8_t(const mi355_attn_params& p, hipStream_t stream) {
  D256Args a;
  a.p = p;
  a.group = p.num_q_heads / p.num_kv_heads;
  a.block_q = kQRows / a.group;
  a.page_shift = __builtin_ctz((unsigned)p.page_size);
  a.k_page_b = (uint32_t)p.k_stride_page; a.k_slot_b = (uint32_t)p.k_stride_slot;      // one byte an element
  a.v_page_b = (uint32_t)p.v_stride_page; a.v_slot_b = (uint32_t)p.v_stride_slot;
  const int qblocks = p.num_tokens / a.block_q + p.num_seqs;   // static upper bound, as for the other Q-block kernels
  static std::atomic<uint64_t> lds_opt_in{0};
  const int rc0 = ensure_dynamic_lds((const void*)prefill_q8_kernel<E5, SW>, kQLds, lds_opt_in, "hipFuncSetAttribute(prefill_q8)");
  if (rc0 != MI355_OK) return rc0;
  hipLaunchKernelGGL((prefill_q8_kernel<E5, SW>), dim3(qblocks * p.num_kv_heads), dim3(256), kQLds, stream, a);
  const int rc = check_hip(hipGetLastError(), "prefill_q8_kernel launch");
  if (rc == MI355_OK) set_kernel_name(SW ? "prefill_mfma_q8_sw" : "prefill_mfma_q8");
  return rc;
}

int launch_prefill_q8(const mi355_attn_params& p, hipStream_t stream) {
  if (!prefill_q8_supported(p)) return MI355_ERR_UNSUPPORTED;
  const bool e5 = p.kv_dtype == MI355_FP8_E5M2;
  if (p.sliding_window > 0) return e5 ? launch_q8_t<true, true>(p, stream) : launch_q8_t<false, true>(p, stream);
  return e5 ? launch_q8_t<true, false>(p, stream) : launch_q8_t<false, false>(p, stream);
}

}  // namespace mi355
