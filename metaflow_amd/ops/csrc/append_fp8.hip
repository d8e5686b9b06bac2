// Append attention over the FP8 page pool for gfx950: Sq new query rows at
// offset pos[b] against the pos[b] + Sq rows that sequence b owns in the
// E4M3 pool of decode_fp8.hip, found through the block table. The third
// cached shape of an FP8 pool (prefill chunks after the first, the verify
// block); decode_fp8.hip covers Sq == 1, attention.hip covers pos == 0.
//
// Include AFTER append.hip (append_paged_lookup, APP_BKV, the merge kernel)
// and decode_fp8.hip (kv8_frag, kv8_u4, KV8_KERNEL).
//
// CONTRACT: that of attn_append_paged_kernel (append.hip), word for word —
// grid (q_tiles * splits, H, B), NW = 1 (32 query rows) or 4 (128), one
// query row per lane, S^T = K·Q^T, online softmax in registers, tile j of
// sequence b = page table[b][j] (readfirstlane), pos a device int32 [B],
// pos[b] < 0 = exact zeros with no table entry read, holes skipped and never
// dereferenced, entries j >= ceil(vis_end / 64) never read, rows >= vis_end
// never loaded, splits == 1 normalises (1 / l guarded) and writes bf16, else
// (o, m, l) partials for attn_append_merge_kernel.
//
// The body is written out here and NOT a switch of attn_append_impl: the
// 1-wave bf16 instantiations sit at 256 VGPRs and must compile to what they
// compile to today.
//
// WHAT IS ITS OWN: where the bytes become bf16. The decode kernel converts
// per wave in registers because each wave owns its own page. Here the NW
// waves of a block share one tile, so the tile is converted ONCE PER BLOCK,
// IN STAGING, and the MFMA loop reads the bf16 panels of attention.hip
// exactly as the bf16 kernel does (frag8_panel rows, ds_read_b64_tr_b16
// columns).
//  * A staging slot is 16 E4M3 bytes, one global_load_dwordx4: 16
//    consecutive d of one row — in the panel layout [d/16][row][16] exactly
//    the 32-byte row segment of one panel, two ds_write_b128. A tile is 512
//    slots per K and per V: 2 + 2 per thread at NW = 4 (prefetched under the
//    MFMAs of the current tile, half the bf16 kernel's registers), 8 + 8 at
//    NW = 1 (staged in place in two groups of 4 + 4).
//  * Lane map: load k of a wave covers the 8 whole rows 8k .. 8k + 7 of the
//    page (1 KiB contiguous): panel = lane >> 3, row = 8k + (lane & 7). The
//    8 lanes of a ds_write_b128 group then own the same panel and 8
//    consecutive rows, 256 contiguous bytes. The two 16-byte halves of a
//    segment are written in swapped order by the lanes of rows 4 .. 7 of the
//    group, so each write instruction of a group covers 8 distinct 16-byte
//    slots mod 128 bytes: every bank once (docs/KERNELS.md, "FP8 paged
//    append", has the arithmetic). The swap selects the raw dwords before
//    the conversion: 4 v_cndmask per slot.
//  * E4M3 -> bf16 is exact (v_cvt_pk_f32_fp8, v_cvt_pk_bf16_f32).
//  * Scales stay off the operands, as in the decode kernel, so a prefill
//    chunk and a decode step of one slot see the same K and V values: the
//    64 K scales (times `scale`) and 64 V scales of the tile sit in a
//    512-byte LDS vector next to the tiles, loaded by threads 0 .. 63 (one
//    256-byte read each, part of the prefetch at NW = 4) and read back as
//    f32x4 in C-register order. s = acc * kscale[row], p * vscale[row] goes
//    into the bf16 pack, l sums the unscaled p.
//  * NW = 1 has no LDS to spare: a 1-wave block with 32768 + 512 bytes
//    fits 4 times into a CU's 160 KiB, one wave per SIMD, where 32768 bytes
//    fit 5 times, the two waves per SIMD the bf16 1-wave kernel is held to.
//    Its 64 lanes ARE the 64 rows of the tile, so lane r keeps the two
//    scales of row r in registers and a lane fetches the scales of its C
//    registers from the row lanes with ds_bpermute (register exchange, no
//    LDS storage): same values, same arithmetic as NW = 4. Multiplying the
//    scales in during staging instead (panel = bf16(e4m3 * scale), the
//    values kv_page_gather_fp8 produces) was built first and measured: the
//    bf16 rounding of K costs |s| * 2^-9 on a score, 1.0e-1 per-row error
//    at scores of +-60 (docs/KERNELS.md).
//  * NaN safety: the pool's unowned bytes may be 0x7F and its scales NaN.
//    Rows >= vis_end and hole tiles stage zero bytes AND zero scales and
//    load neither; masked elements inside the visible range get -inf.

#include "common.h"

static_assert(APP_BKV * ATT_D == KV8_SLAB, "one tile is one FP8 slab");

// A KV8_KERNEL differs from the HIP headers' functions in its target
// features, and the compiler inlines across such a difference only what is
// force-inlined: __shfl, __shfl_xor and __syncthreads on floats would be
// real calls inside the tile loop (37 s_swappc per instantiation, the
// accumulators moved to AGPRs around them). Hence half_pair_max /
// half_pair_sum (attention.hip) for the lane pair, and these two.
DEV float ap8_lane_read(float x, int src_lane) {
  return __int_as_float(
      __builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(x)));
}

// tr_load_bfrags<64> (attention.hip) with the lane part of the address in
// ONE register and k-step, d block and first / second read as instruction
// immediates (tr_read_imm): written with per-read pointers, the 32 read
// addresses of a tile are loop-invariant and held in 32 VGPRs, which the
// 1-wave kernel does not have. tb = lds_addr(tile) + ap8_tr_base(lane);
// waiting is the caller's job.
DEV unsigned int ap8_tr_base(int lane) {
  const int hi = lane >> 5;
  return 2 * (((lane >> 4) & 1) * (APP_BKV * 16) + hi * 8 * 16
              + ((lane >> 2) & 3) * 16 + (lane & 3) * 4);
}

template <int KS>
DEV void ap8_tr_load(BFrag bfr[4], unsigned int tb) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    constexpr int base = 2 * KS * 16 * 16;
    bfr[n].u[0] = tr_read_imm(tb, base + 2 * (n * 2 * (APP_BKV * 16)));
    bfr[n].u[1] =
        tr_read_imm(tb, base + 2 * (n * 2 * (APP_BKV * 16) + 4 * 16));
  }
}

// k-step KS of O += P·V: tile rows 16 KS .. + 15
template <int KS>
DEV void ap8_pv_step(f16f acc_o[4], const bf16x8 pa[4], unsigned int tb) {
  BFrag bfr[4];
  ap8_tr_load<KS>(bfr, tb);
  asm volatile("s_waitcnt lgkmcnt(0)");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_o[n] = mfma32(pa[KS], bfr[n].v, acc_o[n]);
}

DEV void ap8_block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Thread's slot u covers row 8 * (u * NW + wave) + (lane & 7), bytes
// 16 * (lane >> 3) .. + 15. Load slots [U0, U0 + N) of one (page, kv head)
// slab; rows >= ve (tile-local) become zeros and issue no load. row0 is 0
// (see the in-place staging of the 1-wave kernel).
template <int NW, int U0, int N>
DEV void ap8_stage_load(kv8_u4* rk, kv8_u4* rv, const unsigned char* kb,
                        const unsigned char* vb, int row0, int ve) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int row = row0 + 8 * ((U0 + u) * NW + wid) + (lane & 7);
    const int off = row * PG_D + (lane >> 3) * 16;
    const kv8_u4 z = {0u, 0u, 0u, 0u};
    rk[u] = z;
    rv[u] = z;
    if (row < ve) {
      rk[u] = *(const kv8_u4*)(kb + off);
      rv[u] = *(const kv8_u4*)(vb + off);
    }
  }
}

// 16 bytes -> the 16 bf16 of one panel row segment, as the two halves a
// lane writes first and second: `swap` lanes start with the upper one
DEV void ap8_cvt(kv8_u4 w, bool swap, bf16x8& first, bf16x8& second) {
  first = kv8_frag(swap ? w[2] : w[0], swap ? w[3] : w[1]);
  second = kv8_frag(swap ? w[0] : w[2], swap ? w[1] : w[3]);
}

// registers -> the [8][64][16] bf16 panel layout of attention.hip. The
// lane keeps two element offsets (its first and its second half); slot and
// tile are constants on top of them.
template <int NW, int U0, int N>
DEV void ap8_stage_write(short* kp, short* vp, const kv8_u4* rk,
                         const kv8_u4* rv) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const bool swap = (lane >> 2) & 1;
  const int pel = (lane >> 3) * (APP_BKV * 16) + (8 * wid + (lane & 7)) * 16;
  const int pel1 = pel + (swap ? 8 : 0), pel2 = pel + (swap ? 0 : 8);
#pragma unroll
  for (int u = 0; u < N; ++u) {
    constexpr int SLOT = 8 * NW * 16;  // elements between a thread's slots
    bf16x8 first, second;
    ap8_cvt(rk[u], swap, first, second);
    *(bf16x8*)(kp + pel1 + (U0 + u) * SLOT) = first;
    *(bf16x8*)(kp + pel2 + (U0 + u) * SLOT) = second;
    ap8_cvt(rv[u], swap, first, second);
    *(bf16x8*)(vp + pel1 + (U0 + u) * SLOT) = first;
    *(bf16x8*)(vp + pel2 + (U0 + u) * SLOT) = second;
  }
}

// The tile's row scales: thread r < 64 holds those of row r, zero (and no
// load) for rows >= ve. ksb/vsb point at the slab's 64 scales.
DEV void ap8_scale_load(float& ks, float& vs, const float* ksb,
                        const float* vsb, int ve) {
  ks = 0.f;
  vs = 0.f;
  if ((int)threadIdx.x < min(ve, PG_ROWS)) {
    ks = ksb[threadIdx.x];
    vs = vsb[threadIdx.x];
  }
}

// sc[0..63] = kscale * scale, sc[64..127] = vscale
DEV void ap8_scale_write(float* sc, float ks, float vs, float scale) {
  if (threadIdx.x < PG_ROWS) {
    sc[threadIdx.x] = ks * scale;
    sc[PG_ROWS + threadIdx.x] = vs;
  }
}

// Whole tile global -> LDS, in place, in groups of SLOTS slots per thread
// (the fence keeps the compiler from hoisting every load of the tile above
// the first write), and its row scales into ks / vs (ap8_scale_load).
template <int NW, int SLOTS>
DEV void ap8_stage_tile(short* kp, short* vp, float& ks, float& vs,
                        kv8_u4* rk, kv8_u4* rv, const unsigned char* kb,
                        const unsigned char* vb, const float* ksb,
                        const float* vsb, int row0, int ve) {
  constexpr int PER = 8 / NW;
  static_assert(PER == SLOTS || PER == 2 * SLOTS, "one or two groups");
  ap8_scale_load(ks, vs, ksb, vsb, ve);
  ap8_stage_load<NW, 0, SLOTS>(rk, rv, kb, vb, row0, ve);
  ap8_stage_write<NW, 0, SLOTS>(kp, vp, rk, rv);
  if constexpr (PER == 2 * SLOTS) {
    __builtin_amdgcn_sched_barrier(0);
    ap8_stage_load<NW, SLOTS, SLOTS>(rk, rv, kb, vb, row0, ve);
    ap8_stage_write<NW, SLOTS, SLOTS>(kp, vp, rk, rv);
  }
}

// q [B,H,Sq,128] bf16; kpool/vpool [num_pages,Hkv,64,128] E4M3 bytes; ksc/
// vsc [num_pages,Hkv,64] fp32; table int32 [B,table_stride]; pos int32 [B].
// splits == 1: writes o [B,H,Sq,128] bf16.
// splits  > 1: writes o_part [splits,B,H,Sq,128] and ml_part
//              [splits,B,H,Sq,2] fp32 (unnormalised o, running max, sum).
template <int NW>
KV8_KERNEL __launch_bounds__(NW * WAVE)
__attribute__((amdgpu_waves_per_eu(2, 2))) void attn_append_paged_fp8_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ kpool,
    const unsigned char* __restrict__ vpool, const float* __restrict__ ksc,
    const float* __restrict__ vsc, const int* __restrict__ table,
    const int* __restrict__ pos, short* __restrict__ o,
    float* __restrict__ o_part, float* __restrict__ ml_part, int B, int H,
    int Hkv, int Sq, int num_pages, int table_stride, int splits,
    float scale) {
  constexpr int BQ = NW * 32, BKV = APP_BKV, PER = 8 / NW;
  constexpr bool PREFETCH = (NW > 1);
  // where the tile's row scales live: an LDS vector, or (1 wave: lane =
  // row) the registers rks / rvs, read across lanes
  constexpr bool SC_LDS = (NW > 1);
  // staging registers: the whole share with PREFETCH, else half of it
  constexpr int SLOTS = PREFETCH ? PER : PER / 2;
  __shared__ short kp[BKV * ATT_D];
  __shared__ short vp[BKV * ATT_D];
  // row scales of the tile: k (times `scale`), then v. Never referenced
  // (and not allocated) without SC_LDS.
  __shared__ __attribute__((aligned(16))) float sc[2 * PG_ROWS];

  const int qt = blockIdx.x / splits;
  const int sp = blockIdx.x - qt * splits;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hk = h / (H / Hkv);
  const WaveCoord c = wave_coord();
  const int wid = __builtin_amdgcn_readfirstlane(c.wid);
  const int lane = c.lane, l32 = c.l32, hi = c.hi;

  // everything below is bounded by the capacity whatever pos holds
  const int cap = table_stride * BKV;
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

  const int* trow = table + (long long)b * table_stride;
  const unsigned int v_tb = lds_addr(vp) + ap8_tr_base(lane);
  kv8_u4 rk[SLOTS], rv[SLOTS];
  // row scales of thread r < 64. SC_LDS: the prefetched tile's, on their
  // way to `sc`; else those of the tile in LDS, k already times `scale`
  float rks = 0.f, rvs = 0.f;

  // A slab is 64 * 128 BYTES here, so the element offset the lookup
  // returns is the byte offset into the pool, and off / 128 the row offset
  // into the scales. Block-uniform: whether the tile in LDS is a real page.
  bool page_ok;
  {
    long long off;
    int ve;
    append_paged_lookup(trow, t0, num_pages, Hkv, hk, vis_end, page_ok, off,
                        ve);
    ap8_stage_tile<NW, SLOTS>(kp, vp, rks, rvs, rk, rv, kpool + off,
                              vpool + off, ksc + off / PG_D, vsc + off / PG_D,
                              0, ve);
    if constexpr (SC_LDS) ap8_scale_write(sc, rks, rvs, scale);
    else rks *= scale;
  }
  ap8_block_sync();
  for (int j = t0; j < t1; ++j) {
    const bool more = j + 1 < t1;
    // the next tile's page, looked up before its loads are issued
    bool nxt_ok = false;
    long long nxt_off = 0;
    int nxt_ve = 0;
    if (PREFETCH && more) {
      append_paged_lookup(trow, j + 1, num_pages, Hkv, hk, vis_end, nxt_ok,
                          nxt_off, nxt_ve);
      ap8_scale_load(rks, rvs, ksc + nxt_off / PG_D, vsc + nxt_off / PG_D,
                     nxt_ve);
      ap8_stage_load<NW, 0, SLOTS>(rk, rv, kpool + nxt_off, vpool + nxt_off,
                                   0, nxt_ve);
    }

    // block-uniform: a hole contributes no key. wave-uniform causal skip:
    // the tile starts past every horizon of this wave (or the wave holds
    // no real row)
    if (page_ok && wave_on && j * BKV <= wave_hz_max) {
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

      // ---- row scale + horizon mask + in-register online softmax ----
      // lane's value (t, r) is S[my_q][kv = j*64 + t*32 + c_row(r,hi)], and
      // registers 4g .. 4g+3 are the 4 consecutive rows 8g + 4hi .. + 3;
      // the per-element mask only on tiles crossing some row's horizon
      const bool cross = j * BKV + BKV - 1 > wave_hz_min;
      // 1 wave: the row lane of register 4g + i of sub-tile t is 32t + 8g
      // + i + 4hi; the lane part is opaque so that the 64 source lanes are
      // per-tile temporaries (as src0 below)
      int row4 = 4 * hi;
      asm volatile("" : "+v"(row4));
      float pmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 kq;
          if constexpr (SC_LDS) {
            kq = *(const f32x4*)(sc + t * 32 + 8 * g + 4 * hi);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              kq[i] = ap8_lane_read(rks, t * 32 + 8 * g + i + row4);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * g + i;
            float sv = st[t][r] * kq[i];
            if (cross) {
              const int kvg = j * BKV + t * 32 + c_row(r, hi);
              if (kvg > hz) sv = -INFINITY;
            }
            st[t][r] = sv;
            pmax = fmaxf(pmax, sv);
          }
        }
      }
      pmax = half_pair_max(pmax);
      const float newm = fmaxf(m_run, pmax);
      // a row that has seen no key yet keeps m == -inf: subtract 0
      // instead, so exp() gets -inf (-> 0), never -inf - -inf
      const float m_sub = (newm == -INFINITY) ? 0.f : newm;
      const float rescale = __expf(m_run - m_sub);
      m_run = newm;

      // p, its unscaled row sum, and p * vscale[row] for the product
      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 vq;
          if constexpr (SC_LDS) {
            vq = *(const f32x4*)(sc + PG_ROWS + t * 32 + 8 * g + 4 * hi);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              vq[i] = ap8_lane_read(rvs, t * 32 + 8 * g + i + row4);
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float e = __expf(st[t][4 * g + i] - m_sub);
            psum += e;
            st[t][4 * g + i] = e * vq[i];
          }
        }
      }
      psum = half_pair_sum(psum);
      l_run = l_run * rescale + psum;

      // ---- rescale O: the factor of local row c_row(r, hi) is held by
      // the lanes with l32 == that row. c_row(r, hi) + 32 hi is a constant
      // of r plus 36 hi; the lane part goes through an empty asm so that
      // the 16 source lanes are per-tile temporaries, not 16 VGPRs held
      // across the loop ----
      int src0 = 36 * hi;
      asm volatile("" : "+v"(src0));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float f = ap8_lane_read(rescale, c_row(r, 0) + src0);
#pragma unroll
        for (int n = 0; n < 4; ++n) acc_o[n][r] *= f;
      }

      // ---- P -> bf16 A-fragments; PV with transposed V reads ----
      bf16x8 pa[4];
      col_to_afrags<2>(st, pa, hi);
      ap8_pv_step<0>(acc_o, pa, v_tb);
      ap8_pv_step<1>(acc_o, pa, v_tb);
      ap8_pv_step<2>(acc_o, pa, v_tb);
      ap8_pv_step<3>(acc_o, pa, v_tb);
    }

    if (more) {
      ap8_block_sync();  // every wave is done reading the tile
      if (PREFETCH) {
        ap8_stage_write<NW, 0, SLOTS>(kp, vp, rk, rv);
        ap8_scale_write(sc, rks, rvs, scale);
      } else {
        append_paged_lookup(trow, j + 1, num_pages, Hkv, hk, vis_end, nxt_ok,
                            nxt_off, nxt_ve);
        // row0 is 0, but the compiler must not know: with a constant the
        // slots' row offsets and bounds tests are loop-invariant, get
        // hoisted and held in VGPRs across the loop (the trap of
        // append.hip's 1-wave kernel, same remedy)
        int row0 = 0;
        asm volatile("" : "+s"(row0));
        ap8_stage_tile<NW, SLOTS>(kp, vp, rks, rvs, rk, rv, kpool + nxt_off,
                                  vpool + nxt_off, ksc + nxt_off / PG_D,
                                  vsc + nxt_off / PG_D, row0, nxt_ve);
        rks *= scale;
      }
      ap8_block_sync();
    }
    page_ok = nxt_ok;
  }

  // ---- epilogue: the store pattern of the bf16 kernel ----
  if (splits == 1) {
    // a row whose every page is a hole has seen no key: l == 0, o == 0
    const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row_local = c_row(r, hi);
      const float f = ap8_lane_read(inv_l, row_local + 32 * hi);
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
