// Flash attention train kernels for gfx950 (bf16, head dim 128, GQA):
//   attn_fwd_v2_kernel        forward, writes O and lse
//   attn_bwd_delta_kernel     delta = rowsum(dO * O)
//   attn_bwd_dkdv_v2_kernel   dK/dV fp32 partials, one query head per block
//   dkdv_reduce_kernel        sums the G partials per kv head -> bf16
//   attn_bwd_dq_v2_kernel     dQ
// The three MFMA kernels share one structure: 512 threads = 8 waves x 32
// rows, mfma_f32_32x32x16_bf16, and the SWAPPED product S^T = K·Q^T (or
// S = Q·K^T in dkdv) so that each lane's C-register column is its OWN row
// of the wave's operand held in registers. Consequences:
//  * softmax statistics are per-lane scalars: the online softmax is a
//    serial max/sum over the lane's 16 C registers per 32-row sub-tile
//    plus one exchange between the lane halves in the register file
//    (half_pair_max / half_pair_sum) — no cross-lane group reductions,
//    no LDS round-trip for P;
//  * P / dS are, as they stand, the B operand of the TRANSPOSED second
//    product (O^T = V^T·P^T, dQ^T = K^T·dS^T, dV^T = dO^T·P, dK^T =
//    Q^T·dS): acc_to_bfrags packs bf16 pairs and trades halves with
//    v_permlane32_swap, no ds_bpermute in any tile loop. The results
//    come out transposed (d in the registers, the row on the lane); each
//    epilogue turns them back through LDS tiles that are free by then
//    (store_acc_tile_t, store_acc_tile_t_bf16);
//  * LDS holds only the streamed operand tiles, in the dual-use IMAGE A
//    of attn_lds_image.h (8-row x 32-column subtiles, XOR-swizzled),
//    which serves the row-fragment reads (ds_read_b128) and the
//    hardware-transposed fragment reads (ds_read_b64_tr_b16) from one
//    copy, both free of bank conflicts. The 16-wide PANEL layout below
//    remains for the append kernels, the dK/dV V image and the probe;
//  * one block per (256-row tile, head, batch element) on a 1-D grid,
//    dispatched heavy causal tiles first (block_coord).
// col_to_afrags and store_acc_tile (the untransposed forms) remain for
// the append kernels (col_to_afrags) and the layout probe (both).
//
// MFMA 32x32x16 layouts (probed on HW by dbg_mfma32_kernel; the panel /
// transposed-read / col_to_afrags chain by dbg_attn_layout_kernel, the
// image / acc_to_bfrags chain by dbg_attn_image_kernel):
//  A (32x16): lane holds A[lane&31][(lane>>5)*8 + i]
//  B (16x32): lane holds B[(lane>>5)*8 + i][lane&31]
//  C (32x32): col = lane&31, row = c_row(reg, lane>>5)
//
// Shapes: q/o/dout [B,H,S,128], k/v [B,Hkv,S,128], lse/delta [B,H,S] fp32,
// S % 256 == 0 (the Python wrapper zero-pads unaligned causal seqlens:
// end-padded keys are causally masked for every real query row).

#include "common.h"
#include "attn_lds_image.h"

#define ATT_D 128

typedef __attribute__((ext_vector_type(16))) float f16f;

DEV f16f mfma32(bf16x8 a, bf16x8 b, f16f c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// wave / lane coordinates every kernel here uses: lane = 32*hi + l32.
// (dq and dkdv compute the same four values inline: taking them from
// here changed how the compiler narrows their epilogue address math.)
struct WaveCoord {
  int wid, lane, l32, hi;
};

DEV WaveCoord wave_coord() {
  WaveCoord c;
  c.wid = threadIdx.x / WAVE;
  c.lane = threadIdx.x & (WAVE - 1);
  c.l32 = c.lane & 31;
  c.hi = c.lane >> 5;
  return c;
}

// row of the 32x32 C tile held in register r of a lane in half-wave hi
DEV int c_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// pack two fp32 into one u32 of two bf16 (lo, hi): single
// v_cvt_pk_bf16_f32 on gfx950 (RNE) — the manual shift/round sequence
// was ~12 VALU ops and the P->A-fragment repack runs twice per subtile
// in every attention kernel
DEV unsigned int pack_bf2(float lo, float hi) {
  union { __hip_bfloat162 h; unsigned int u; } c;
  c.h = __float22bfloat162_rn(make_float2(lo, hi));
  return c.u;
}

// Turn a per-lane C-tile column (st[NT][16]: lane holds X[row][mycol] for
// rows c_row(r, hi) of NT 32-row sub-tiles) into MFMA A-fragments with
// m = mycol and k = the row dimension: pack bf16 pairs, exchange with the
// partner half-wave (shfl_xor 32), assemble 2*NT k-steps of 16 rows.
template <int NT>
DEV void col_to_afrags(const f16f* st, bf16x8* pa, int hi) {
  unsigned int pk[NT * 8], xp[NT * 8];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j2 = 0; j2 < 8; ++j2)
      pk[t * 8 + j2] = pack_bf2(st[t][j2 * 2], st[t][j2 * 2 + 1]);
#pragma unroll
  for (int i = 0; i < NT * 8; ++i) xp[i] = __shfl_xor(pk[i], 32, WAVE);
#pragma unroll
  for (int ks = 0; ks < NT * 2; ++ks) {
    union {
      unsigned int w[4];
      bf16x8 v;
    } u;
    if (hi == 0) {
      u.w[0] = pk[4 * ks];
      u.w[1] = pk[4 * ks + 1];
      u.w[2] = xp[4 * ks];
      u.w[3] = xp[4 * ks + 1];
    } else {
      u.w[0] = xp[4 * ks + 2];
      u.w[1] = xp[4 * ks + 3];
      u.w[2] = pk[4 * ks + 2];
      u.w[3] = pk[4 * ks + 3];
    }
    pa[ks] = u.v;
  }
}

// ================= panel layout + hardware transpose reads =================
// A [ROWS][128] bf16 tile stored as 8 panels of [ROWS][16]: element
// (row, d) lives at (d>>4)*ROWS*16 + row*16 + (d&15). Properties:
//  * staging from row-major global is pure vec8 -> vec8 (no scalar scatter);
//  * A-fragment reads (row fixed per lane, 8 contiguous d) are one
//    16-byte read: panel (d0>>4), offset row*16 + (d0&8);
//  * B-fragments with K = the row dimension come from ds_read_b64_tr_b16
//    (tr_load_bfrags) — no transposed copy of the tile is ever made.

template <int ROWS, int BLOCK>
DEV void stage_panel(short* dst, const short* src,
                     long long src_row_stride) {
  constexpr int TOT = ROWS * 16;  // vec8 slots
#pragma unroll
  for (int it = 0; it < (TOT + BLOCK - 1) / BLOCK; ++it) {
    const int idx = it * BLOCK + threadIdx.x;
    if (idx < TOT) {
      const int r = idx % ROWS, c8 = idx / ROWS;
      bf16x8 v = *(const bf16x8*)(src + r * src_row_stride + c8 * 8);
      *(bf16x8*)(dst + (c8 >> 1) * (ROWS * 16) + r * 16 + (c8 & 1) * 8) =
          v;
    }
  }
}

template <int ROWS>
DEV bf16x8 frag8_panel(const short* tile, int row, int d0) {
  return *(const bf16x8*)(tile + (d0 >> 4) * (ROWS * 16) + row * 16
                          + (d0 & 15));
}

// issue one tr-read: returns 2 VGPRs holding rows (base_q .. base_q+3) at
// this lane's column; caller must s_waitcnt lgkmcnt + sched_barrier before
// consuming (inline-asm DS reads are invisible to the compiler's waitcnt
// insertion).
DEV unsigned long long tr_read(const short* lds_ptr) {
  // generic pointers to __shared__ carry the LDS offset in the low 32
  // bits; ds_* instructions take that 32-bit address
  unsigned int addr = (unsigned int)(unsigned long long)lds_ptr;
  unsigned long long out;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(out) : "v"(addr));
  return out;
}

union BFrag {
  unsigned long long u[2];
  bf16x8 v;
};

// Issue the 8 transposed reads that give this lane its four B-fragments
// (n = 0..3: d columns n*32 + l32) for the 16 tile rows row0 .. row0+15
// of a [ROWS][128] panel tile; K = the row dimension. Waiting is the
// CALLER's job (s_waitcnt lgkmcnt + sched_barrier before the MFMAs), so
// callers can pipeline several groups with counted waits.
//
// ds_read_b64_tr_b16 semantics: each lane loads 64b at its OWN address;
// the HW transposes 16-bit elements within each 16-lane group (a [4][16]
// tile): elem = base + (l&15) + j*16 + (l>>4)*64 walks column (l&15) of
// that subtile, which in panel storage is exactly 4 consecutive rows at
// one d-column. To make lane l = 32*hi + l32 RECEIVE rows row0+hi*8+j at
// column n*32+l32, lane l must LOAD the 4 elements of row
// row0+hi*8+((l>>2)&3) at col offset 4*(l&3) of panel 2n + ((l>>4)&1);
// the second read covers rows +4..+7.
template <int ROWS>
DEV void tr_load_bfrags(BFrag bfr[4], const short* tile, int row0,
                        int lane, int hi) {
  const int tr_lane_off = (((lane >> 2) & 3) * 16) + (lane & 3) * 4;
  const int tr_panel = ((lane >> 4) & 1) * (ROWS * 16);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int base = n * 2 * (ROWS * 16) + tr_panel
                     + (row0 + hi * 8) * 16 + tr_lane_off;
    bfr[n].u[0] = tr_read(tile + base);
    bfr[n].u[1] = tr_read(tile + base + 4 * 16);
  }
}

// ================= dual-use image A (attn_lds_image.h) ====================
// The streamed tiles of the three train kernels. Addresses are BYTES and
// come from the header's functions: a lane keeps two row-read bases (k-step
// parity) and two transposed-read bases (first / second read of a
// fragment); tile row group, k-step and d block are instruction
// immediates.

// 32-bit LDS address of a __shared__ object (low half of the generic
// pointer), the form ds_* instructions take
DEV unsigned int lds_addr(const void* p) {
  return (unsigned int)(unsigned long long)p;
}

// transposed read at a lane base plus a compile-time byte offset (imm
// must fold to a constant: call it from fully unrolled code only). Same
// waiting rules as tr_read.
DEV unsigned long long tr_read_imm(unsigned int base, int imm) {
  unsigned long long out;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(out)
               : "v"(base), "i"(imm));
  return out;
}

// row fragment: row 32t + l32, d = 16s + 8hi .. +7; rb0 / rb1 are the
// lane's lds_img::row_base_a(lane, 0 / 1)
DEV bf16x8 img_row_frag(const short* tile, int rb0, int rb1, int t, int s) {
  return *(const bf16x8*)((const char*)tile + ((s & 1) ? rb1 : rb0)
                          + lds_img::row_imm_a(t, s));
}

// the 8 transposed reads of k-step ks (tile rows 16ks .. 16ks+15): this
// lane's four fragments, n = 0..3: d columns 32n + l32, rows 16ks + 8hi +
// (0..7). tb0 / tb1 = lds_addr(tile) + lds_img::tr_base_a(lane, 0 / 1).
// Waiting is the caller's job, as with tr_load_bfrags.
DEV void img_tr_load(BFrag bfr[4], unsigned int tb0, unsigned int tb1,
                     int ks) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    bfr[n].u[0] = tr_read_imm(tb0, lds_img::tr_imm_a(ks, n));
    bfr[n].u[1] = tr_read_imm(tb1, lds_img::tr_imm_a(ks, n));
  }
}

// stage a [ROWS][128] row-major global tile into image A, lanes walking
// rows (stage_panel's thread map)
template <int ROWS, int BLOCK>
DEV void stage_image(short* dst, const short* src,
                     long long src_row_stride) {
  constexpr int TOT = ROWS * 16;  // 16-byte chunks
#pragma unroll
  for (int it = 0; it < (TOT + BLOCK - 1) / BLOCK; ++it) {
    const int idx = it * BLOCK + threadIdx.x;
    if (idx < TOT) {
      const int r = lds_img::stage_walk_row(ROWS, idx);
      const int ch = lds_img::stage_walk_ch(ROWS, idx);
      bf16x8 v = *(const bf16x8*)(src + r * src_row_stride + ch * 8);
      *(bf16x8*)((char*)dst + lds_img::off_a(r, ch)) = v;
    }
  }
}

// ---- accumulator-tile epilogue ----
DEV void put_elem(short* p, float x) { *p = f2bf(x); }
DEV void put_elem(float* p, float x) { *p = x; }

// Store a wave's 32 x 128 accumulator tile (acc[n]: C tile of d columns
// n*32..n*32+31) to rows row0.. of a row-major [rows][128] array starting
// at dst[off0]. With ROW_SCALE, row i is first multiplied by the value of
// `lane_scale` held by the lane whose l32 == i (the swapped structure
// keeps per-row scalars in the lane that owns the row). Used by the
// layout probe; the train kernels accumulate the
// transposed product and store through store_acc_tile_t /
// store_acc_tile_t_bf16 below. tr_load_bfrags above serves the append
// kernels and the probe; the train kernels read image A (img_tr_load; dkdv
// keeps an open-coded copy of that addressing).
template <bool ROW_SCALE, typename T>
DEV void store_acc_tile(T* dst, long long off0, int row0, const f16f acc[4],
                        int l32, int hi, float lane_scale = 1.f) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row_local = c_row(r, hi);
    float f = 1.f;
    if (ROW_SCALE) f = __shfl(lane_scale, row_local + 32 * hi, WAVE);
    const long long obase = off0 + (long long)(row0 + row_local) * ATT_D;
#pragma unroll
    for (int n = 0; n < 4; ++n)
      put_elem(dst + obase + n * 32 + l32,
               ROW_SCALE ? acc[n][r] * f : acc[n][r]);
  }
}

// ---- accumulator tile as the next MFMA's B operand ----
// C tile (column on the lane, rows in the registers) -> the two bf16 B
// fragments (k-steps of 16 rows) of a product that sums over its rows.
// Packed pairwise, lane half hi holds rows 16s + {0..3, 8..11} + 4hi of
// step s; two v_permlane32_swap per step (a register-file half exchange,
// no LDS) trade the lower half's rows 8..11 for the upper half's rows
// 4..7, so element j of lane half hi is row 16s + 8hi + j: the NATURAL k
// order. That keeps every product in the k slot it has in the
// untransposed form (O = P·V, dQ = dS·K, dV = P^T·dO, dK = dS^T·Q), so the
// fp32 sums are bit-identical to it; feeding the packed registers
// unswapped (permuted k order) is also a valid operand but changes the
// order in which an MFMA adds its 16 products.
DEV void acc_to_bfrags(const f16f& x, bf16x8* pb) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    unsigned int w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[i] = pack_bf2(x[8 * s + 2 * i], x[8 * s + 2 * i + 1]);
    union {
      unsigned int w[4];
      bf16x8 v;
    } u;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      auto r = __builtin_amdgcn_permlane32_swap(w[i], w[2 + i], false,
                                                false);
      u.w[i] = r[0];
      u.w[2 + i] = r[1];
    }
    pb[s] = u.v;
  }
}

// max / sum of a value over the two lanes l32 and l32 + 32, in the
// register file: swapping x with itself leaves the lower half's value in
// r[0] and the upper half's in r[1] on BOTH lanes, so no select follows.
DEV float half_pair_max(float x) {
  const unsigned int u = __float_as_uint(x);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

DEV float half_pair_sum(float x) {
  const unsigned int u = __float_as_uint(x);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Lanes of one wave exchanging data through LDS: the hardware runs a
// wave's DS instructions in order, but the compiler's per-lane alias
// analysis may move a read above the partner lane's write unless fenced.
DEV void lds_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Store a wave's TRANSPOSED accumulators (acc[n][r] = X[row = l32][d =
// n*32 + c_row(r, hi)], the result of the transposed second product) as
// 32 bf16 rows of a row-major [rows][128] array, NB 32-column blocks per
// pass through `tw`, NB * 2 KiB of LDS that only this wave touches.
// A lane's 4 consecutive registers are 4 consecutive d: one 8-byte write
// into 16-byte slot (d >> 3) ^ (row & (SLOTS - 1)) of its row; the rows
// then leave as 16 bytes per lane, NB * 64 contiguous bytes per row.
// With ROW_SCALE every element is first multiplied by the lane's own
// `lane_scale` (the lane IS the row here, no broadcast).
template <int NB, bool ROW_SCALE>
DEV void store_acc_tile_t_bf16(short* dst, long long off0, short* tw,
                               const f16f acc[4], int lane,
                               float lane_scale = 1.f) {
  constexpr int SLOTS = NB * 4;   // 16-byte slots per row and pass
  constexpr int ROWLEN = NB * 32;  // shorts per row and pass
  const int l32 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int p = 0; p < 4 / NB; ++p) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n = p * NB + nb;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w[j] = f2bf(ROW_SCALE ? acc[n][4 * g + j] * lane_scale
                                : acc[n][4 * g + j]);
        const int slot = (nb * 4 + g) ^ (l32 & (SLOTS - 1));
        *(bf16x4*)(tw + l32 * ROWLEN + slot * 8 + hi * 4) = w;
      }
    }
    lds_wave_fence();
#pragma unroll
    for (int i = 0; i < SLOTS / 2; ++i) {
      const int row = i * (64 / SLOTS) + lane / SLOTS;
      const int c = lane & (SLOTS - 1);
      const bf16x8 v = *(const bf16x8*)(tw + row * ROWLEN
                                        + ((c ^ (row & (SLOTS - 1))) * 8));
      *(bf16x8*)(dst + off0 + (long long)row * ATT_D + p * ROWLEN + c * 8) =
          v;
    }
    if (p + 1 < 4 / NB) lds_wave_fence();
  }
}

// ---- block order ----
// The three MFMA kernels run on a ONE-dimensional grid of T*H*B blocks
// (T = S/256 tiles) and take their (tile, h, b) from the block id here.
// Under the causal mask a block's work grows 16-fold with its tile
// index, one 512-thread block fills a CU, and blocks go out in id order,
// dealt round-robin over the 8 XCDs. So the id order decides two things:
//  * which XCD gets which tiles. With the tile index fastest (the former
//    (T, H, B) grid) XCD x ran tiles x and x + 8 of every head: 10 units
//    of work on one XCD, 24 on another;
//  * how long the tail is: the last blocks dispatched run alone.
// Order: b slowest, then the tile from heavy to light, h fastest. Every
// XCD then runs every tile (H % 8 == 0 deals each tile's heads evenly),
// the heavy tiles go first, and the heads of a GQA group at one tile run
// at the same time. `rank` counts tiles in dispatch order; each kernel
// maps it to its heaviest-first tile index. Scalar arithmetic only.
struct BlockCoord {
  int rank, h, b;
};

DEV BlockCoord block_coord(int T, int H) {
  const int bid = blockIdx.x;
  const int per_b = T * H;
  BlockCoord c;
  c.b = bid / per_b;
  const int r = bid - c.b * per_b;
  c.rank = r / H;
  c.h = r - c.rank * H;
  return c;
}

// ============================ FORWARD ======================================
// One block per (q tile, h, b) in heavy-first order (block_coord), 8 waves
// x 32 q rows; each lane keeps its own q row in registers (8 x bf16x8)
// and streams 64-row K/V tiles through LDS.
// LDS: K and V tiles in image A, double-buffered = 2 x 2 x 16 KiB = 64 KiB.
//
// Q ROW ON THE LANE, BOTH PRODUCTS. S^T = K·Q^T leaves the lane's q row
// of scores in its registers (kv on the rows), which is already the
// B-operand shape of the TRANSPOSED second product O^T(d x q) +=
// V^T(d x kv) · P^T(kv x q): acc_to_bfrags turns P into B fragments in the
// register file, and the transposed reads of the V tile supply V^T as
// the A operand, in the same k slots as O = P·V, so O is bit-identical to
// that form. The accumulators hold d on the rows and q on the lane: the
// online-softmax rescale and the final 1/l are multiplies by the lane's
// own scalar, and nothing in the tile loop crosses lanes through LDS.
// The epilogue transposes each wave's tile through the (by then free)
// K/V buffers so O leaves as whole 256-byte rows.

template <int BLOCK>  // BLOCK = 512 (8 waves)
__global__ __launch_bounds__(512) void attn_fwd_v2_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse, int B, int H, int Hkv, int S, float scale,
    int causal) {
  constexpr int BQ = 256, BKV = 64;  // 8 waves x 32 q rows
  // double-buffered K/V tiles in image A (attn_lds_image.h): staging is
  // pure vec8 writes, K A-fragments are conflict-free 16-byte row reads,
  // V^T A-fragments come from ds_read_b64_tr_b16 of the same copy. Stage
  // j+1 overlaps compute on j (async-stage split).
  __shared__ short kp[2][BKV * ATT_D];
  __shared__ short vp[2][BKV * ATT_D];

  const BlockCoord bc = block_coord(S / BQ, H);
  const int qb = S / BQ - 1 - bc.rank;  // most kv tiles first
  const int h = bc.h;
  const int b = bc.b;
  const int hk = h / (H / Hkv);
  const WaveCoord c = wave_coord();
  const int wid = c.wid, lane = c.lane, l32 = c.l32, hi = c.hi;

  const int my_qrow = qb * BQ + wid * 32 + l32;  // this lane's q row
  const long long hoff = ((long long)b * H + h) * S;
  const long long qoff = (hoff + qb * BQ) * ATT_D;
  const long long kvoff0 = ((long long)b * Hkv + hk) * S * ATT_D;

  // Q row in registers: q_reg[s] = Q[my_qrow][s*16 + hi*8 .. +8]
  bf16x8 q_reg[8];
  {
    const short* qrow = q + (hoff + my_qrow) * ATT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      q_reg[s] = *(const bf16x8*)(qrow + s * 16 + hi * 8);
  }

  float m_run = -INFINITY;
  float l_run = 0.f;
  f16f acc_o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_o[n] = (f16f){};

  // per-thread staging slices: 2 x bf16x8 of K and of V per tile
  const int tid = threadIdx.x;
  bf16x8 stg_k[2], stg_v[2];
  int stg_r[2], stg_c8[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = u * BLOCK + tid;
    stg_r[u] = lds_img::stage16_row(idx);
    stg_c8[u] = lds_img::stage16_ch(idx);
  }
  // image addresses (bytes): the thread's staging chunk (slot u is 32 rows
  // = 8192 bytes further), the lane's row-read and transposed-read bases
  const int stg_off = lds_img::stage16_addr_a(tid);
  const int rb0 = lds_img::row_base_a(lane, 0);
  const int rb1 = lds_img::row_base_a(lane, 1);
  const unsigned int tb0 = lds_addr(&vp[0][0]) + lds_img::tr_base_a(lane, 0);
  const unsigned int tb1 = lds_addr(&vp[0][0]) + lds_img::tr_base_a(lane, 1);

  // global loads and LDS writes of a tile are split so the loads for
  // tile j+1 are in flight during the MFMAs on tile j; kept as macros
  // because they close over the staging registers above
#define MFX_STAGE_LOAD(jj)                                               \
  {                                                                      \
    const short* kb_ = k + kvoff0 + (long long)(jj) * BKV * ATT_D;       \
    const short* vb_ = v + kvoff0 + (long long)(jj) * BKV * ATT_D;       \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                      \
      stg_k[u] = *(const bf16x8*)(kb_ + stg_r[u] * ATT_D + stg_c8[u] * 8);\
      stg_v[u] = *(const bf16x8*)(vb_ + stg_r[u] * ATT_D + stg_c8[u] * 8);\
    }                                                                    \
  }

#define MFX_STAGE_WRITE(buf)                                             \
  {                                                                      \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                      \
      const int pel_ = stg_off + u * 8192;                               \
      *(bf16x8*)((char*)kp[buf] + pel_) = stg_k[u];                      \
      *(bf16x8*)((char*)vp[buf] + pel_) = stg_v[u];                      \
    }                                                                    \
  }

  const int kv_tiles =
      causal ? (qb * BQ + BQ) / BKV : S / BKV;  // causal bound incl diag
  MFX_STAGE_LOAD(0);
  MFX_STAGE_WRITE(0);
  __syncthreads();
  for (int j = 0; j < kv_tiles; ++j) {
    const int cur = j & 1;
    if (j + 1 < kv_tiles) MFX_STAGE_LOAD(j + 1);  // issue loads early

    // wave-uniform skip: this wave's rows are all below the tile's kv
    // range (fully masked) — staging + barrier still run below
    const bool active = !causal || (j * BKV <= qb * BQ + wid * 32 + 31);
    if (active) {

    // ---- S^T = K (64x128) @ Q^T: two 32-kv sub-tiles ----
    f16f st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = (f16f){};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        bf16x8 kf = img_row_frag(kp[cur], rb0, rb1, t, s);
        st[t] = mfma32(kf, q_reg[s], st[t]);
      }
    }

    // ---- scale + causal mask + in-register online softmax ----
    // lane's value (t, r) is S[my_qrow][kv = j*64 + t*32 + c_row(r,hi)]
    // The mask is a pass of its own behind a block-uniform (scalar)
    // branch: only the block's 4 diagonal tiles can lose an element; all
    // others run no compare and no select. (Narrowing the predicate to
    // the wave's own diagonal measured no faster: docs/KERNELS.md.)
    const bool diag = causal && (j * BKV + BKV > qb * BQ);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] *= scale;
    if (diag) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kvg = j * BKV + t * 32 + c_row(r, hi);
          if (kvg > my_qrow) st[t][r] = -INFINITY;
        }
    }
    float pmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) pmax = fmaxf(pmax, st[t][r]);
    pmax = half_pair_max(pmax);
    const float newm = fmaxf(m_run, pmax);
    const float rescale = __expf(m_run - newm);
    m_run = newm;

    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float e = __expf(st[t][r] - newm);
        st[t][r] = e;
        psum += e;
      }
    psum = half_pair_sum(psum);
    l_run = l_run * rescale + psum;

    // ---- rescale O^T: the lane is the q row, the factor is its own ----
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_o[n][r] *= rescale;

    // ---- P -> bf16 B-fragments in the register file ----
    bf16x8 pb[4];
    acc_to_bfrags(st[0], pb);
    acc_to_bfrags(st[1], pb + 2);

    // ---- PV: O^T(128d x 32q) += V^T(128d x 64kv) @ P^T(64kv x 32q) ----
    // V^T A-fragments via hardware transpose of the image (img_tr_load:
    // two lane bases, k-step and d block as immediates)
    {
      const unsigned int tbc0 = tb0 + cur * (BKV * ATT_D * 2);
      const unsigned int tbc1 = tb1 + cur * (BKV * ATT_D * 2);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        BFrag bfr[4];
        img_tr_load(bfr, tbc0, tbc1, ks);
        asm volatile("s_waitcnt lgkmcnt(0)");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_o[n] = mfma32(bfr[n].v, pb[ks], acc_o[n]);
      }
    }
    }  // active

    if (j + 1 < kv_tiles) MFX_STAGE_WRITE(cur ^ 1);
    __syncthreads();
  }
#undef MFX_STAGE_LOAD
#undef MFX_STAGE_WRITE

  // ---- epilogue: O /= l (the lane's own), write bf16 + lse. Every wave
  // is past the loop's last barrier, so the K/V buffers are free: each
  // wave transposes its tile through its own 8 KiB of them ----
  float inv_l = 1.f / l_run;
  short* tw = (wid < 4 ? &kp[0][0] : &vp[0][0]) + (wid & 3) * (32 * ATT_D);
  store_acc_tile_t_bf16<4, true>(o, qoff + (long long)wid * 32 * ATT_D, tw,
                                 acc_o, lane, inv_l);
  if (hi == 0)
    lse[hoff + my_qrow] = m_run + __logf(l_run);
}

// ===================== BACKWARD: delta preprocess ==========================
// delta[row] = rowsum(dO[row] * O[row]); one wave per row, 2 elems/lane.
// A separate tiny kernel so both MFMA backward kernels stay
// elementwise-free.
__global__ void attn_bwd_delta_kernel(const short* __restrict__ dout,
                                      const short* __restrict__ o,
                                      float* __restrict__ delta,
                                      long long rows) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const long long row = (long long)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (row >= rows) return;
  const short* dr = dout + row * ATT_D;
  const short* orow = o + row * ATT_D;
  float s = bf2f(dr[lane]) * bf2f(orow[lane])
            + bf2f(dr[lane + 64]) * bf2f(orow[lane + 64]);
  s = wave_sum(s);
  if (lane == 0) delta[row] = s;
}

// ===================== BACKWARD: dQ ========================================
// One block per (q tile, h, b) in heavy-first order (block_coord), 8 waves
// x 32 q rows. Swapped structure: lane's C-column is its OWN q row, so
// lse/delta are per-lane scalars and dS^T is, as it stands, the B operand
// of the transposed product dQ^T(d x q) += K^T(d x kv) · dS^T(kv x q)
// (acc_to_bfrags, natural k order: bit-identical to dQ = dS·K). Q and dO
// rows live in registers. LDS: K and V tiles in image A, double-buffered as in
// the forward (loads for tile j+1 issue before the MFMAs on tile j, the
// LDS writes follow them, one barrier per tile): the first pair is the
// static 2 x 16 KiB, the second pair the 32 KiB of dynamic LDS
// (DQ_DYN_LDS at the launch site). The K tile serves both S^T
// (A-fragments, row reads) and the K^T A-fragments (transposed reads).
// The epilogue transposes each wave's dQ^T tile through its 4 KiB of
// the static tiles, two 64-column halves.

// dynamic LDS of the dq kernel: its second K/V tile pair, K then V
extern __shared__ __attribute__((aligned(16))) short dq_kv2[];
#define DQ_DYN_LDS (2 * 64 * ATT_D * 2)

template <int BLOCK>
__global__ __launch_bounds__(512) void attn_bwd_dq_v2_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dq, int B, int H, int Hkv, int S, float scale,
    int causal) {
  constexpr int BQ = 256, BKV = 64;
  __shared__ short kp[BKV * ATT_D];    // K image
  __shared__ short vp[BKV * ATT_D];    // V image

  const BlockCoord bc = block_coord(S / BQ, H);
  const int qb = S / BQ - 1 - bc.rank;  // most kv tiles first
  const int h = bc.h;
  const int b = bc.b;
  const int hk = h / (H / Hkv);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int l32 = lane & 31;
  const int hi = lane >> 5;

  const int my_qrow = qb * BQ + wid * 32 + l32;
  const long long hoff = ((long long)b * H + h) * S;
  const long long qoff = (hoff + qb * BQ) * ATT_D;
  const long long kvoff0 = ((long long)b * Hkv + hk) * S * ATT_D;

  bf16x8 q_reg[8], do_reg[8];
  {
    const short* qrow = q + (hoff + my_qrow) * ATT_D;
    const short* drow = dout + (hoff + my_qrow) * ATT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      q_reg[s] = *(const bf16x8*)(qrow + s * 16 + hi * 8);
      do_reg[s] = *(const bf16x8*)(drow + s * 16 + hi * 8);
    }
  }
  const float my_lse = lse[hoff + my_qrow];
  const float my_del = delta[hoff + my_qrow];

  f16f acc_dq[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_dq[n] = (f16f){};

  // per-thread staging slices, 2 x bf16x8 of K and of V per tile; buffer 0
  // is (kp, vp), buffer 1 the dynamic pair. Macros as in the forward.
  const int tid = threadIdx.x;
  bf16x8 stg_k[2], stg_v[2];
  // image addresses (bytes), as in the forward
  const int stg_off = lds_img::stage16_addr_a(tid);
  const int rb0 = lds_img::row_base_a(lane, 0);
  const int rb1 = lds_img::row_base_a(lane, 1);
  const int trl0 = lds_img::tr_base_a(lane, 0);
  const int trl1 = lds_img::tr_base_a(lane, 1);
  const int wid_s = __builtin_amdgcn_readfirstlane(threadIdx.x) / WAVE;
#define MFX_DQ_LOAD(jj)                                                  \
  {                                                                      \
    const short* kb_ = k + kvoff0 + (long long)(jj) * BKV * ATT_D;       \
    const short* vb_ = v + kvoff0 + (long long)(jj) * BKV * ATT_D;       \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                      \
      const int idx_ = u * BLOCK + tid;                                  \
      stg_k[u] = *(const bf16x8*)(kb_ + (idx_ / 16) * ATT_D + (idx_ % 16) * 8);\
      stg_v[u] = *(const bf16x8*)(vb_ + (idx_ / 16) * ATT_D + (idx_ % 16) * 8);\
    }                                                                    \
  }
#define MFX_DQ_WRITE(buf)                                                \
  {                                                                      \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                      \
      const int pel_ = stg_off + u * 8192;                               \
      *(bf16x8*)((char*)((buf) ? dq_kv2 : kp) + pel_) = stg_k[u];        \
      *(bf16x8*)((char*)((buf) ? dq_kv2 + BKV * ATT_D : vp) + pel_) =    \
          stg_v[u];                                                      \
    }                                                                    \
  }
  const int kv_tiles = causal ? (qb * BQ + BQ) / BKV : S / BKV;
  MFX_DQ_LOAD(0);
  MFX_DQ_WRITE(0);
  __syncthreads();
  for (int j = 0; j < kv_tiles; ++j) {
    const int cur = j & 1;
    const short* kpc = cur ? dq_kv2 : kp;
    const short* vpc = cur ? dq_kv2 + BKV * ATT_D : vp;
    if (j + 1 < kv_tiles) MFX_DQ_LOAD(j + 1);  // issue loads early
    // wave-uniform skip of tiles above this wave's rows; staging and the
    // barrier still run below
    if (!(causal && j * BKV > qb * BQ + wid * 32 + 31)) {

    // per 32-kv sub-tile: S^T, dP^T, dS, dQ — keeps live regs low
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f16f st = (f16f){}, dpt = (f16f){};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        bf16x8 kf = img_row_frag(kpc, rb0, rb1, t, s);
        bf16x8 vf = img_row_frag(vpc, rb0, rb1, t, s);
        st = mfma32(kf, q_reg[s], st);
        dpt = mfma32(vf, do_reg[s], dpt);
      }
      // dS = P * (dP - delta) * scale, P = exp(S*scale - lse), causal.
      // The mask sits behind a wave-uniform (scalar) branch: only a
      // sub-tile whose last key lies above the wave's first q row can
      // lose an element.
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = __expf(st[r] * scale - my_lse);
      if (causal && j * BKV + t * 32 + 31 > qb * BQ + wid_s * 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kvg = j * BKV + t * 32 + c_row(r, hi);
          if (kvg > my_qrow) st[r] = 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st[r] = st[r] * (dpt[r] - my_del) * scale;
      // dQ^T(128d x 32q) += K^T(128d x 32kv) @ dS^T(32kv x 32q)
      bf16x8 pb[2];
      acc_to_bfrags(st, pb);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        BFrag bfr[4];
        img_tr_load(bfr, lds_addr(kpc) + trl0, lds_addr(kpc) + trl1,
                    t * 2 + ks);
        asm volatile("s_waitcnt lgkmcnt(0)");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_dq[n] = mfma32(bfr[n].v, pb[ks], acc_dq[n]);
      }
    }
    }  // active
    if (j + 1 < kv_tiles) MFX_DQ_WRITE(cur ^ 1);
    __syncthreads();
  }
#undef MFX_DQ_LOAD
#undef MFX_DQ_WRITE

  // epilogue: C row = d, col = q local; every wave is past the loop's last
  // barrier, so the static tiles are free for the transpose.
  short* tw = (wid < 4 ? kp : vp) + (wid & 3) * (32 * 64);
  store_acc_tile_t_bf16<2, false>(dq, qoff + (long long)wid * 32 * ATT_D,
                                  tw, acc_dq, lane);
}

// ===================== BACKWARD: dK/dV =====================================
// One block per (kv tile, h, b) in heavy-first order (block_coord) — one
// Q-HEAD per block, mirroring the dq kernel's structure (which measures 2.2x more TF/s than the round-1 dkdv that
// looped all G q-heads inside a (S/256, Hkv, B) grid: 4x fewer blocks
// with a skewed causal trapezoid starved/imbalanced the chip). Each
// block accumulates its head's (dK, dV) contribution in registers and
// writes FP32 PARTIALS laid out [B, H, S, D]; dkdv_reduce_kernel sums
// the G partials per kv head and converts to bf16 — numerically
// identical to the old in-register fp32 accumulation across g. 8 waves
// x 32 kv rows. LDS: Q and dO tiles in image A (2 x 16 KiB) + 64 lse + 64
// delta floats = 33280 bytes.
//
// KEY ON THE LANE. S = Q·K^T and dP = dO·V^T come out as C[q][kv]: the
// lane is the kv row, the 16 registers are q rows. That is already the
// B-operand shape of the TRANSPOSED products
//   dV^T(d x kv) += dO^T(d x q) · P(q x kv),  dK^T += Q^T · dS,
// so P and dS need the pairwise bf16 pack and a half exchange between the
// lane halves in the register file (acc_to_bfrags) — no ds_bpermute, no
// LDS. The exchange restores the natural k order, which keeps the
// results bit-identical to the dV = P^T·dO form; tests/
// test_attn_dkdv_exact_gpu.py checks the operand pairing with exact
// integers.
// The accumulators hold d on the rows and kv on the lane; the epilogue
// transposes them through the (by then free) Q/dO tiles so the partials
// keep their [B,H,S,D] rows and 128-byte store segments.
//
// K/V RESIDENCY. The wave's 32 K rows and 32 V rows (64 VGPRs as B
// fragments) are loaded ONCE before the q sweep. Plain loads are not
// enough: the compiler treats them as rematerialisable and, at the
// 256-VGPR limit, puts all 32 global loads back inside the tile loop
// (the earlier version of this kernel did exactly that under a comment
// that claimed residency). The empty asm after the loads makes the values
// opaque, so they either stay in registers or show up as spills, which
// tests/test_attn_kernel_resources.py forbids; tests/test_dkdv_loop_asm.py
// counts the loop's global loads.
//
// Code generation here is fragile (register limit): the coordinates, the
// transposed-read addressing and the epilogue stay open-coded rather than
// going through wave_coord() / img_tr_load / store_acc_tile.

// Store a wave's transposed accumulators (acc[n][r] = X[kv = l32][d =
// n*32 + c_row(r, hi)]) as 32 rows of a row-major [rows][128] fp32 array:
// one 32 x 32 block at a time through the wave's own 4 KiB of LDS, XOR-
// swizzled so both the column writes and the row reads are conflict-free.
// Each store instruction covers two rows x 128 contiguous bytes.
DEV void store_acc_tile_t(float* dst, long long off0, float* tw,
                          const f16f acc[4], int l32, int hi) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dl = (r & 3) + 8 * (r >> 2) + 4 * hi;
      tw[l32 * 32 + (dl ^ l32)] = acc[n][r];
    }
    lds_wave_fence();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 2 * i + hi;
      dst[off0 + (long long)row * ATT_D + n * 32 + l32] =
          tw[row * 32 + (l32 ^ row)];
    }
    lds_wave_fence();
  }
}

// dynamic LDS of the dkdv kernel: the block's 256 V rows, 64 KiB
// (DKDV_DYN_LDS at the launch site); the static arrays end 16-byte aligned
extern __shared__ __attribute__((aligned(16))) short dkdv_v_img[];
#define DKDV_DYN_LDS (256 * ATT_D * 2)

template <int BLOCK>
__global__ __launch_bounds__(512) void attn_bwd_dkdv_v2_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    float* __restrict__ dk_part, float* __restrict__ dv_part,
    int B, int H, int Hkv, int S, float scale, int causal) {
  constexpr int BKVB = 256, BQ2 = 64;
  // Q and dO tiles in image A, one array so that a transposed read
  // reaches either tile from one lane base by an immediate
  __shared__ short qdo[2 * BQ2 * ATT_D];
  short* const qp = qdo;                  // Q image
  short* const dop = qdo + BQ2 * ATT_D;   // dO image
  __shared__ float lse_s[BQ2];
  __shared__ float del_s[BQ2];

  const BlockCoord bc = block_coord(S / BKVB, H);
  const int kvb = bc.rank;            // most q tiles first
  const int h = bc.h;                 // q head
  const int b = bc.b;
  const int G = H / Hkv;
  const int hk = h / G;               // kv head this block feeds
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int l32 = lane & 31;
  const int hi = lane >> 5;

  const int my_kvrow = kvb * BKVB + wid * 32 + l32;
  const long long kvoff =
      (((long long)b * Hkv + hk) * S + kvb * BKVB) * ATT_D;

  // this lane's K row as B fragments in registers and its V row in the
  // dynamic LDS image, both resident for the whole q sweep (K/V
  // RESIDENCY above). The image is [wave][8 panels][32 rows][16]: a
  // lane's fragment s sits at s*512 + lane*8 shorts, so every wave read
  // is 1 KiB contiguous, and each lane reads back only what it wrote
  // itself — no barrier.
  bf16x8 kr[8];
  short* vimg = dkdv_v_img + wid * (32 * ATT_D) + lane * 8;
  {
    const short* krow = k + kvoff + (long long)(wid * 32 + l32) * ATT_D;
    const short* vrow = v + kvoff + (long long)(wid * 32 + l32) * ATT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      kr[s] = *(const bf16x8*)(krow + s * 16 + hi * 8);
      *(bf16x8*)(vimg + s * 512) = *(const bf16x8*)(vrow + s * 16 + hi * 8);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(kr[s]));
  }

  f16f acc_dk[4], acc_dv[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    acc_dk[n] = (f16f){};
    acc_dv[n] = (f16f){};
  }

  // image addresses (bytes): the lane's row-read bases and its
  // transposed-read bases as LDS addresses into qp; dop lies DOP_REL
  // bytes from qp
  const int rb0 = lds_img::row_base_a(lane, 0);
  const int rb1 = lds_img::row_base_a(lane, 1);
  const unsigned int tb0 = lds_addr(qp) + lds_img::tr_base_a(lane, 0);
  const unsigned int tb1 = lds_addr(qp) + lds_img::tr_base_a(lane, 1);
  constexpr int DOP_REL = BQ2 * ATT_D * 2;
  // scalar copy of the wave index for the wave-uniform mask branch
  const int wid_s = __builtin_amdgcn_readfirstlane(threadIdx.x) / WAVE;

  const long long hoff = ((long long)b * H + h) * S;
  const int jq0 = causal ? (kvb * BKVB) / BQ2 : 0;
  const int nq = S / BQ2;
  for (int jq = jq0; jq < nq; ++jq) {
    __syncthreads();
    const short* qsrc = q + (hoff + (long long)jq * BQ2) * ATT_D;
    const short* dsrc = dout + (hoff + (long long)jq * BQ2) * ATT_D;
    stage_image<BQ2, BLOCK>(qp, qsrc, ATT_D);
    stage_image<BQ2, BLOCK>(dop, dsrc, ATT_D);
    if (threadIdx.x < BQ2) {
      lse_s[threadIdx.x] = lse[hoff + jq * BQ2 + threadIdx.x];
      del_s[threadIdx.x] = delta[hoff + jq * BQ2 + threadIdx.x];
    }
    __syncthreads();
    // wave-uniform skip: all of this wave's kv rows above every q row
    if (causal && jq * BQ2 + BQ2 - 1 < kvb * BKVB + wid * 32) continue;

    // per 32-q sub-tile: S, dP, P/dS, dV^T, dK^T — keeps live regs low
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f16f st = (f16f){}, dpt = (f16f){};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        bf16x8 qf = img_row_frag(qp, rb0, rb1, t, s);
        bf16x8 df = img_row_frag(dop, rb0, rb1, t, s);
        bf16x8 vf = *(const bf16x8*)(vimg + s * 512);
        st = mfma32(qf, kr[s], st);
        dpt = mfma32(df, vf, dpt);
      }
      // P (into st) with causal mask q >= kv; dS (into dpt). lse/delta
      // come as f32x4 GROUP loads: the per-element lse_s[qrl] reads were
      // 64 scalar ds_read_b32 per tile (the dq kernel holds its lse in
      // a register). qrl = t*32 + c_row(r, hi), so r = g*4+j walks
      // 4 consecutive floats at t*32 + 8g + 4hi.
      // The mask is a pass of its own behind a wave-uniform (scalar) branch: only a
      // sub-tile whose first q row lies below the wave's last key can
      // lose an element.
      const bool edge =
          causal && jq * BQ2 + t * 32 < kvb * BKVB + wid_s * 32 + 31;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q0l = t * 32 + g * 8 + 4 * hi;
        const f32x4 lv = *(const f32x4*)&lse_s[q0l];
        const f32x4 dl = *(const f32x4*)&del_s[q0l];
        float p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          p[j] = __expf(st[g * 4 + j] * scale - lv[j]);
        if (edge) {
          asm volatile("");
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (jq * BQ2 + q0l + j < my_kvrow) p[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = g * 4 + j;
          st[r] = p[j];
          dpt[r] = p[j] * (dpt[r] - dl[j]) * scale;
        }
      }
      // dV^T(128d x 32kv) += dO^T(128d x 32q) @ P(32q x 32kv), then
      // dK^T += Q^T @ dS — FOUR transposed-read groups (one 16-q k-step
      // each), software-pipelined with COUNTED waits: group g+1's 8 DS
      // reads issue before waiting on group g (DS returns in order, so
      // lgkmcnt(8) = "the earlier 8 are done"), so the transpose-read
      // latency of every group but the last hides under the previous
      // group's MFMAs.
      bf16x8 pb[2], pbk[2];
      acc_to_bfrags(st, pb);
      BFrag bfr[2][4];
      // image addressing as img_tr_load (open-coded copy: the lane bases
      // tb0 / tb1 point into qp, group g reads tile dop (DOP_REL further)
      // for g < 2 and qp after, k-step 2t + (g & 1)); the fragments serve as the A
      // operand dO^T / Q^T
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int imm = DOP_REL + lds_img::tr_imm_a(2 * t, n);
        bfr[0][n].u[0] = tr_read_imm(tb0, imm);
        bfr[0][n].u[1] = tr_read_imm(tb1, imm);
      }
      acc_to_bfrags(dpt, pbk);  // VALU under the first DS group
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cur = g & 1;
        if (g < 3) {
          const int rel = (g + 1 < 2) ? DOP_REL : 0;
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int imm = rel + lds_img::tr_imm_a(2 * t + ((g + 1) & 1), n);
            bfr[cur ^ 1][n].u[0] = tr_read_imm(tb0, imm);
            bfr[cur ^ 1][n].u[1] = tr_read_imm(tb1, imm);
          }
          asm volatile("s_waitcnt lgkmcnt(8)");
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)");
        }
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 bop = (g < 2) ? pb[g] : pbk[g - 2];
        f16f* acc = (g < 2) ? acc_dv : acc_dk;
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[n] = mfma32(bfr[cur][n].v, bop, acc[n]);
      }
    }
  }

  // epilogue: fp32 partials at [b, h, kv row, d]. Every wave is done with
  // the Q/dO tiles after the barrier; each then transposes through its
  // own 4 KiB of them.
  __syncthreads();
  float* tw = (float*)(wid < 4 ? qp : dop) + (wid & 3) * 1024;
  const long long poff =
      (hoff + (long long)kvb * BKVB + wid * 32) * ATT_D;
  store_acc_tile_t(dk_part, poff, tw, acc_dk, l32, hi);
  store_acc_tile_t(dv_part, poff, tw, acc_dv, l32, hi);
}

// Sum the G per-q-head fp32 partials into the kv head's bf16 (dK, dV).
// Memory-bound; vectorized f32x4 loads, grid-stride.
__global__ void dkdv_reduce_kernel(const float* __restrict__ dk_part,
                                   const float* __restrict__ dv_part,
                                   short* __restrict__ dk,
                                   short* __restrict__ dv,
                                   long long n4_kv, int G,
                                   long long head_elems) {
  // n4_kv = B*Hkv*S*D/4. Flat kv vec4-index i4 -> kv slot (b*Hkv + hk);
  // its G partials live at heads slot*G + g of the [B, H, S, D] buffer
  // (h = hk*G + g).
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i4 < n4_kv; i4 += stride) {
    const long long i = i4 * 4;
    const long long slot = i / head_elems;
    const long long rem = i - slot * head_elems;
    const float* kp = dk_part + slot * G * head_elems + rem;
    const float* vp = dv_part + slot * G * head_elems + rem;
    f32x4 ks = *(const f32x4*)kp;
    f32x4 vs = *(const f32x4*)vp;
    for (int g = 1; g < G; ++g) {
      const f32x4 k2 = *(const f32x4*)(kp + (long long)g * head_elems);
      const f32x4 v2 = *(const f32x4*)(vp + (long long)g * head_elems);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ks[j] += k2[j];
        vs[j] += v2[j];
      }
    }
    bf16x4 ko, vo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ko[j] = f2bf(ks[j]);
      vo[j] = f2bf(vs[j]);
    }
    *(bf16x4*)(dk + i) = ko;
    *(bf16x4*)(dv + i) = vo;
  }
}
