// Append attention for gfx950: Sq new query rows at offset pos[b] against
// the pos[b] + Sq rows already in the KV cache (bf16, head dim 128, GQA).
// This is the shape of speculative verification (Sq = k+1) and of every
// chunk after the first in chunked prefill; attention.hip covers pos == 0
// and decode.hip covers Sq == 1. One kernel body, attn_append_impl, serves
// the dense cache (attn_append_kernel) and the paged one
// (attn_append_paged_kernel): what differs sits behind `PAGED`.
//
// Include AFTER attention.hip and paged.hip: the kernel is built from
// attention.hip's helpers (mfma32, wave_coord, c_row, col_to_afrags,
// frag8_panel, tr_load_bfrags) and has the forward kernel's structure —
// swapped product S^T = K·Q^T, each lane owns one query row in registers,
// online softmax in registers, P -> A-fragments in-register, V B-fragments
// by transposed LDS reads. What differs from the forward:
//  * the cache is read at its ALLOCATION stride (Lmax), no slicing copies;
//  * query row i of sequence b sees cache rows 0 .. pos[b]+i, with pos a
//    DEVICE int32 [B]: the host never reads it;
//  * Sq is arbitrary: lanes whose row is >= Sq load a clamped (valid) row,
//    compute a finite duplicate and store nothing. Every cross-lane
//    exchange in this structure (shfl_xor 32, the row-owner broadcast)
//    stays within one query row, so those lanes cannot leak into real rows;
//  * cache rows >= min(pos[b] + end of this q tile, Lmax) are never
//    loaded: staging writes zeros for them. That keeps every read inside
//    the allocation (a 64-row tile may straddle Lmax) and keeps stale or
//    uninitialised rows (NaN) out of the P·V product, where 0 * NaN would
//    otherwise poison the row;
//  * the KV range is split as in decode.hip: grid (q_tiles * splits, H, B),
//    each split writes unnormalised fp32 partials (o, m, l) per query row,
//    attn_append_merge_kernel combines them. With splits, a query row may
//    see NO key of a split whose other rows do (its horizon lies before
//    the split): m stays -inf, and the rescale / probabilities are guarded
//    so that -inf - -inf never reaches exp(); the merge gives such
//    partials weight 0 without reading them;
//  * with splits == 1 the kernel normalises and writes bf16 itself.
//
// Two block sizes: NW = 1 (32 query rows, the verify block) and NW = 4
// (128 query rows, the prefill chunk). LDS: one K and one V panel tile,
// 2 x 16 KiB. NW = 4 prefetches the next tile into registers (4 + 4
// bf16x8 per thread) under the MFMAs of the current one; NW = 1 would
// need 16 + 16 bf16x8 per lane for that, so it stages in place, in two
// groups of 8 + 8, and relies on the resident blocks of a CU (two waves
// per SIMD, which every instantiation is held to) to cover the latency.
//
// PAGED: the rows that sequence b owns live in the page pool and are found
// through the block table (paged.hip). A page is PG_ROWS = 64 rows and the
// K/V tile is APP_BKV = 64 rows, so tile j of sequence b IS page
// table[b][j] — one table lookup per tile, uniform across the block. What
// differs from the dense instantiation:
//  * the K/V base of tile j is (table[b][j] * Hkv + hk) * 64 * 128 into
//    the pool [num_pages, Hkv, 64, 128]. The entry goes through
//    readfirstlane, so page and base live in scalar registers. The staging
//    helpers take the page as their slab, with row0 = 0 and a tile-local
//    vis_end;
//  * the capacity is table_stride * 64 in place of Lmax;
//  * entry j is read only for j < ceil(vis_end / 64), and an entry that
//    is negative or >= num_pages is never dereferenced: its tile is
//    staged as zeros and skipped, so it contributes no key (the
//    semantics of attn_decode_paged). A query row may therefore see no
//    key at all: the splits == 1 epilogue guards 1 / l and writes zeros;
//  * pos[b] < 0 marks a sequence that takes no part (as in
//    kv_page_write): no table entry is read, and its output rows are
//    exactly zero — written here with splits == 1, by the merge (weight-0
//    partials) otherwise.
// Rows >= vis_end inside the last page are zero-staged and never loaded,
// table entries past the last needed page are never read: the dense
// NaN-safety argument, unchanged. Same tile order, same split rule, same
// arithmetic: on identical rows the two instantiations sum in the same
// order.
//
// The body is shared WHOLE. Both 1-wave instantiations sit at the 256-VGPR
// limit of two waves per SIMD, and moving a PART of such a kernel (its loop
// body) into a common helper reschedules it; one force-inlined body whose
// differences are compile-time switches does not (KERNELS.md, "Fragile
// code generation").

#include "common.h"

#define APP_BKV 64

static_assert(APP_BKV == PG_ROWS, "one append K/V tile must be one page");
static_assert(ATT_D == PG_D, "head dim of the pool");

// Staging is split into a load and a write so that the loads of tile j+1
// can be in flight under the MFMAs of tile j. Thread t's slot u is vec8
// number idx = u * BLOCK + t of the [64][16] tile: 16 threads cover one
// 256-byte row, so a wave's load instruction reads 4 full rows.
//
// Load slots [U0, U0 + N) of rows [row0, row0 + 64) of one (b, kv head)
// cache slab into registers; rows >= vis_end become zeros and issue no
// load.
template <int NW, int U0, int N>
DEV void append_stage_load(bf16x8* rk, bf16x8* rv, const short* kb,
                           const short* vb, int row0, int vis_end) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int idx = (U0 + u) * (NW * WAVE) + threadIdx.x;
    const int row = row0 + (idx >> 4);
    const long long off = (long long)row * ATT_D + (idx & 15) * 8;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    rk[u] = z;
    rv[u] = z;
    if (row < vis_end) {
      rk[u] = *(const bf16x8*)(kb + off);
      rv[u] = *(const bf16x8*)(vb + off);
    }
  }
}

// registers -> the [8][64][16] panel layout of attention.hip
template <int NW, int U0, int N>
DEV void append_stage_write(short* kp, short* vp, const bf16x8* rk,
                            const bf16x8* rv) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int idx = (U0 + u) * (NW * WAVE) + threadIdx.x;
    const int r = idx >> 4, c8 = idx & 15;
    const int pel = (c8 >> 1) * (APP_BKV * 16) + r * 16 + (c8 & 1) * 8;
    *(bf16x8*)(kp + pel) = rk[u];
    *(bf16x8*)(vp + pel) = rv[u];
  }
}

// Whole tile, global -> LDS, in groups of SLOTS slots per thread. The
// scheduling fence between groups keeps the compiler from hoisting every
// load of the tile above the first write (16 + 16 bf16x8 = 128 VGPRs per
// lane at NW = 1, which spills at two waves per SIMD).
template <int NW, int SLOTS>
DEV void append_stage_tile(short* kp, short* vp, bf16x8* rk, bf16x8* rv,
                           const short* kb, const short* vb, int row0,
                           int vis_end) {
  constexpr int PER = 16 / NW;
  static_assert(PER % SLOTS == 0, "slot groups must tile the thread's share");
  if constexpr (PER >= SLOTS) {
    append_stage_load<NW, 0, SLOTS>(rk, rv, kb, vb, row0, vis_end);
    append_stage_write<NW, 0, SLOTS>(kp, vp, rk, rv);
  }
  if constexpr (PER >= 2 * SLOTS) {
    __builtin_amdgcn_sched_barrier(0);
    append_stage_load<NW, SLOTS, SLOTS>(rk, rv, kb, vb, row0, vis_end);
    append_stage_write<NW, SLOTS, SLOTS>(kp, vp, rk, rv);
  }
  static_assert(PER <= 2 * SLOTS, "at most two groups");
}

// Page of tile j of one sequence (trow = its table row): whether it is a
// real pool page, its element offset for kv head hk, and the tile-local
// vis_end. A hole (entry < 0 or outside the pool) gives offset 0 with a
// vis_end of 0: every row is zero-staged, nothing is loaded. The entry
// is uniform across the block; readfirstlane keeps all three results in
// scalar registers.
DEV void append_paged_lookup(const int* trow, int j, int num_pages, int Hkv,
                             int hk, int vis_end, bool& ok, long long& off,
                             int& ve) {
  const int page = __builtin_amdgcn_readfirstlane(trow[j]);
  ok = page >= 0 && page < num_pages;
  off = ok ? ((long long)page * Hkv + hk) * (PG_ROWS * PG_D) : 0;
  ve = ok ? vis_end - j * PG_ROWS : 0;
}

// The one kernel body. Dense: kc/vc [B,Hkv,Lmax,128], table null,
// num_pages and table_stride unused. PAGED: kc/vc are the pool
// [num_pages,Hkv,64,128], table int32 [B,table_stride], Lmax unused.
template <int NW, bool PAGED>
DEV void attn_append_impl(
    const short* __restrict__ q, const short* __restrict__ kc,
    const short* __restrict__ vc, const int* __restrict__ table,
    const int* __restrict__ pos, short* __restrict__ o,
    float* __restrict__ o_part, float* __restrict__ ml_part, int B, int H,
    int Hkv, int Sq, int Lmax, int num_pages, int table_stride, int splits,
    float scale) {
  constexpr int BQ = NW * 32, BKV = APP_BKV, PER = 16 / NW;
  constexpr bool PREFETCH = (NW > 1);
  // staging registers: the whole share with PREFETCH, else half of it
  constexpr int SLOTS = PREFETCH ? PER : PER / 2;
  __shared__ short kp[BKV * ATT_D];
  __shared__ short vp[BKV * ATT_D];

  const int qt = blockIdx.x / splits;
  const int sp = blockIdx.x - qt * splits;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hk = h / (H / Hkv);
  const WaveCoord c = wave_coord();
  const int wid = __builtin_amdgcn_readfirstlane(c.wid);
  const int lane = c.lane, l32 = c.l32, hi = c.hi;

  // everything below is bounded by the capacity whatever pos holds
  const int cap = PAGED ? table_stride * BKV : Lmax;
  const int p_raw = pos[b];
  const int p = min(max(p_raw, 0), cap);
  const int q0 = qt * BQ;
  const int vis_end = min(p + min(q0 + BQ, Sq), cap);
  const int n_tiles = (vis_end + BKV - 1) / BKV;
  const int tps = (n_tiles + splits - 1) / splits;
  const int t0 = sp * tps;
  const int t1 = min(n_tiles, t0 + tps);

  const int qw0 = q0 + wid * 32;         // first query row of this wave
  const int my_q = qw0 + l32;
  const bool q_ok = my_q < Sq;
  const int my_qc = min(my_q, Sq - 1);   // clamped: always a real row
  const long long row_g = ((long long)b * H + h) * Sq;  // + query row
  const long long R = (long long)B * H * Sq;

  if constexpr (PAGED) {
    if (p_raw < 0) {
      // the sequence takes no part: zeros, and no table entry is read
      if (q_ok) {
        if (splits == 1) {
          // the lane pair (hi = 0, 1) of a row writes 64 columns each
          const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          short* orow = o + (row_g + my_q) * ATT_D + hi * 64;
#pragma unroll
          for (int n = 0; n < 8; ++n) *(bf16x8*)(orow + n * 8) = z;
        } else if (hi == 0) {
          const long long pm = ((long long)sp * R + row_g + my_q) * 2;
          ml_part[pm] = -INFINITY;
          ml_part[pm + 1] = 0.f;
        }
      }
      return;
    }
  }

  if (t0 >= t1) {
    // empty split (only with splits > 1): weight-0 partial, o unread
    if (q_ok && hi == 0) {
      const long long pm = ((long long)sp * R + row_g + my_q) * 2;
      ml_part[pm] = -INFINITY;
      ml_part[pm + 1] = 0.f;
    }
    return;
  }

  // last visible key of this lane's row, and the wave's extremes
  const int hz = min(p + my_qc, cap - 1);
  const bool wave_on = qw0 < Sq;
  const int wave_hz_max = min(p + min(qw0 + 31, Sq - 1), cap - 1);
  const int wave_hz_min = min(p + min(qw0, Sq - 1), cap - 1);

  // Q row in registers: q_reg[s] = Q[my_qc][s*16 + hi*8 .. +8]
  bf16x8 q_reg[8];
  {
    const short* qrow = q + (row_g + my_qc) * ATT_D;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      q_reg[s] = *(const bf16x8*)(qrow + s * 16 + hi * 8);
  }

  float m_run = -INFINITY;
  float l_run = 0.f;
  f16f acc_o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_o[n] = (f16f){};

  // dense: the (b, kv head) slab; paged: the sequence's table row
  const long long kvoff =
      PAGED ? 0 : ((long long)b * Hkv + hk) * Lmax * ATT_D;
  const short* kb = kc + kvoff;
  const short* vb = vc + kvoff;
  const int* trow = PAGED ? table + (long long)b * table_stride : nullptr;
  bf16x8 rk[SLOTS], rv[SLOTS];

  // block-uniform: whether the tile in LDS is a real page (dense: always)
  bool page_ok = true;
  if constexpr (PAGED) {
    long long off;
    int ve;
    append_paged_lookup(trow, t0, num_pages, Hkv, hk, vis_end, page_ok, off,
                        ve);
    append_stage_tile<NW, SLOTS>(kp, vp, rk, rv, kc + off, vc + off, 0, ve);
  } else {
    append_stage_tile<NW, SLOTS>(kp, vp, rk, rv, kb, vb, t0 * BKV, vis_end);
  }
  __syncthreads();
  for (int j = t0; j < t1; ++j) {
    const bool more = j + 1 < t1;
    // paged: the next tile's page, looked up before its loads are issued
    bool nxt_ok = !PAGED;
    long long nxt_off = 0;
    int nxt_ve = 0;
    if (PREFETCH && more) {
      if constexpr (PAGED) {
        append_paged_lookup(trow, j + 1, num_pages, Hkv, hk, vis_end, nxt_ok,
                            nxt_off, nxt_ve);
        append_stage_load<NW, 0, SLOTS>(rk, rv, kc + nxt_off, vc + nxt_off,
                                        0, nxt_ve);
      } else {
        append_stage_load<NW, 0, SLOTS>(rk, rv, kb, vb, (j + 1) * BKV,
                                        vis_end);
      }
    }

    // block-uniform: a hole contributes no key. wave-uniform causal
    // skip: the tile starts past every horizon of this wave (or the wave
    // holds no real row)
    if ((!PAGED || page_ok) && wave_on && j * BKV <= wave_hz_max) {
      // ---- S^T = K (64x128) @ Q^T: two 32-kv sub-tiles ----
      f16f st[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        st[t] = (f16f){};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          bf16x8 kf = frag8_panel<BKV>(kp, t * 32 + l32, s * 16 + hi * 8);
          st[t] = mfma32(kf, q_reg[s], st[t]);
        }
      }

      // ---- scale + horizon mask + in-register online softmax ----
      // lane's value (t, r) is S[my_q][kv = j*64 + t*32 + c_row(r,hi)];
      // the per-element mask only on tiles crossing some row's horizon
      const bool cross = j * BKV + BKV - 1 > wave_hz_min;
      float pmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float sv = st[t][r] * scale;
          if (cross) {
            const int kvg = j * BKV + t * 32 + c_row(r, hi);
            if (kvg > hz) sv = -INFINITY;
          }
          st[t][r] = sv;
          pmax = fmaxf(pmax, sv);
        }
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, WAVE));
      const float newm = fmaxf(m_run, pmax);
      // a row that has seen no key yet keeps m == -inf: subtract 0
      // instead, so exp() gets -inf (-> 0), never -inf - -inf
      const float m_sub = (newm == -INFINITY) ? 0.f : newm;
      const float rescale = __expf(m_run - m_sub);
      m_run = newm;

      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float e = __expf(st[t][r] - m_sub);
          st[t][r] = e;
          psum += e;
        }
      psum += __shfl_xor(psum, 32, WAVE);
      l_run = l_run * rescale + psum;

      // ---- rescale O: the factor of local row c_row(r, hi) is held by
      // the lanes with l32 == that row ----
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float f = __shfl(rescale, c_row(r, hi) + 32 * hi, WAVE);
#pragma unroll
        for (int n = 0; n < 4; ++n) acc_o[n][r] *= f;
      }

      // ---- P -> bf16 A-fragments; PV with transposed V reads ----
      bf16x8 pa[4];
      col_to_afrags<2>(st, pa, hi);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        BFrag bfr[4];
        tr_load_bfrags<BKV>(bfr, vp, ks * 16, lane, hi);
        asm volatile("s_waitcnt lgkmcnt(0)");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_o[n] = mfma32(pa[ks], bfr[n].v, acc_o[n]);
      }
    }

    if (more) {
      __syncthreads();  // every wave is done reading the tile
      if (PREFETCH) {
        append_stage_write<NW, 0, SLOTS>(kp, vp, rk, rv);
      } else if constexpr (PAGED) {
        append_paged_lookup(trow, j + 1, num_pages, Hkv, hk, vis_end,
                            nxt_ok, nxt_off, nxt_ve);
        // row0 is 0, but the compiler must not know: with a constant
        // row0 every slot's row offset is loop-invariant, gets hoisted
        // and held in VGPRs across the loop, and this instantiation
        // (256 VGPRs, like the dense one) spills the V read addresses.
        // An opaque scalar zero keeps the dense kernel's per-tile
        // address arithmetic.
        int row0 = 0;
        asm volatile("" : "+s"(row0));
        append_stage_tile<NW, SLOTS>(kp, vp, rk, rv, kc + nxt_off,
                                     vc + nxt_off, row0, nxt_ve);
      } else {
        append_stage_tile<NW, SLOTS>(kp, vp, rk, rv, kb, vb, (j + 1) * BKV,
                                     vis_end);
      }
      __syncthreads();
    }
    page_ok = nxt_ok;
  }

  // ---- epilogue: the store pattern of store_acc_tile, plus the row
  // guard (rows >= Sq store nothing) ----
  if (splits == 1) {
    // dense: key 0 is visible to every row, so l_run > 0. paged: a row
    // whose every page is a hole has seen no key: l == 0, o == 0
    const float inv_l = (!PAGED || l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row_local = c_row(r, hi);
      const float f = __shfl(inv_l, row_local + 32 * hi, WAVE);
      if (qw0 + row_local < Sq) {
        const long long obase = (row_g + qw0 + row_local) * ATT_D;
#pragma unroll
        for (int n = 0; n < 4; ++n)
          o[obase + n * 32 + l32] = f2bf(acc_o[n][r] * f);
      }
    }
  } else {
    const long long pbase = (long long)sp * R + row_g;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row_local = c_row(r, hi);
      if (qw0 + row_local < Sq) {
        const long long obase = (pbase + qw0 + row_local) * ATT_D;
#pragma unroll
        for (int n = 0; n < 4; ++n)
          o_part[obase + n * 32 + l32] = acc_o[n][r];
      }
    }
    if (q_ok && hi == 0) {
      const long long pm = (pbase + my_q) * 2;
      ml_part[pm] = m_run;
      ml_part[pm + 1] = l_run;
    }
  }
}

// q [B,H,Sq,128]; kc/vc [B,Hkv,Lmax,128]; pos int32 [B].
// splits == 1: writes o [B,H,Sq,128] bf16.
// splits  > 1: writes o_part [splits,B,H,Sq,128] and ml_part
//              [splits,B,H,Sq,2] fp32 (unnormalised o, running max, sum).
template <int NW>
__global__ __launch_bounds__(NW * WAVE)
__attribute__((amdgpu_waves_per_eu(2, 2))) void attn_append_kernel(
    const short* __restrict__ q, const short* __restrict__ kc,
    const short* __restrict__ vc, const int* __restrict__ pos,
    short* __restrict__ o, float* __restrict__ o_part,
    float* __restrict__ ml_part, int B, int H, int Hkv, int Sq, int Lmax,
    int splits, float scale) {
  attn_append_impl<NW, false>(q, kc, vc, nullptr, pos, o, o_part, ml_part, B,
                              H, Hkv, Sq, Lmax, 0, 0, splits, scale);
}

// As above over the page pool: kpool/vpool [num_pages,Hkv,64,128]; table
// int32 [B,table_stride].
template <int NW>
__global__ __launch_bounds__(NW * WAVE)
__attribute__((amdgpu_waves_per_eu(2, 2))) void attn_append_paged_kernel(
    const short* __restrict__ q, const short* __restrict__ kpool,
    const short* __restrict__ vpool, const int* __restrict__ table,
    const int* __restrict__ pos, short* __restrict__ o,
    float* __restrict__ o_part, float* __restrict__ ml_part, int B, int H,
    int Hkv, int Sq, int num_pages, int table_stride, int splits,
    float scale) {
  attn_append_impl<NW, true>(q, kpool, vpool, table, pos, o, o_part, ml_part,
                             B, H, Hkv, Sq, 0, num_pages, table_stride,
                             splits, scale);
}

// Merge the split partials: one wave per query row, lane owns 2 of the
// 128 columns. A partial with m == -inf (empty split, or a row whose
// horizon lies before the split) has weight 0 and its o is not read.
__global__ __launch_bounds__(256) void attn_append_merge_kernel(
    const float* __restrict__ o_part, const float* __restrict__ ml_part,
    short* __restrict__ o, long long R, int splits) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long row =
      (long long)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
  if (row >= R) return;
  float m_all = -INFINITY;
  for (int sp = 0; sp < splits; ++sp)
    m_all = fmaxf(m_all, ml_part[((long long)sp * R + row) * 2]);
  float l_all = 0.f, o0 = 0.f, o1 = 0.f;
  for (int sp = 0; sp < splits; ++sp) {
    const long long pr = (long long)sp * R + row;
    const float m_s = ml_part[pr * 2];
    if (m_s == -INFINITY) continue;
    const float f = __expf(m_s - m_all);
    l_all += f * ml_part[pr * 2 + 1];
    const f32x2 ov = *(const f32x2*)(o_part + pr * ATT_D + 2 * lane);
    o0 += f * ov[0];
    o1 += f * ov[1];
  }
  const float inv = l_all > 0.f ? 1.f / l_all : 0.f;
  o[row * ATT_D + 2 * lane] = f2bf(o0 * inv);
  o[row * ATT_D + 2 * lane + 1] = f2bf(o1 * inv);
}
