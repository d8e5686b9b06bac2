// FP8 paged KV cache for gfx950: the E4M3 page format, the scatter that
// quantises new K/V rows into it, and a GQA-packed MFMA flash-decode that
// reads it.
//
// Format (fixed, shared with models/kv_cache.py PagedKVCache in FP8 mode):
//  * pools k_pages / v_pages: [num_pages, Hkv, 64, 128] bytes, OCP E4M3
//    (float8_e4m3fn) — a (page, kv head) slab is 64 rows of 128 bytes;
//  * scales k_scales / v_scales: [num_pages, Hkv, 64] fp32, one per cached
//    row and kv head. A row x[128] is quantised once, when it is written:
//    amax = max|x|, scale = amax / 448, inv = amax > 0 ? 448 / amax : 0,
//    byte = RNE-E4M3(clamp(x * inv, -448, 448)); value = e4m3(byte) * scale.
//    A zero row stores zero bytes and scale 0;
//  * block table: as in paged.hip.
//
// DECODE. The bf16 paged decode (decode.hip) runs one query head per block,
// so a GQA group of G = H / Hkv heads fetches every page G times. Here a
// block is one (split, KV HEAD, sequence) and serves all G heads from one
// pass over the pages:
//  * grid (splits, Hkv, B), 4 waves; wave w takes pages u0 + w, u0 + w + 4,
//    .. of the split (a split is whole pages, the rule of decode.hip);
//  * S^T = K · Q^T with mfma_f32_32x32x16_bf16: the 64 rows of the page are
//    the A operand (two 32-row halves), the G heads the B operand. Lane
//    (l32, hi) owns head min(l32, G - 1): columns >= G compute a finite
//    duplicate of the last head and store nothing. The scores of a head lie
//    in its lane's registers, so the online softmax is the forward kernel's:
//    serial over 32 registers plus one half_pair_max / half_pair_sum;
//  * K goes global -> registers, no LDS, k-permuted as in moe.hip: lane
//    (row l32 of half t, half-wave hi) reads the 64 contiguous bytes
//    d = 64 hi .. 64 hi + 63 of its row as four 16-byte loads, the two
//    half-waves consume whole 128-byte rows. Fragment s (8 bytes) is
//    d = 64 hi + 8 s .. + 7, converted E4M3 -> fp32 -> bf16 in registers
//    (exact: 3 mantissa bits) right before its MFMA. The matching Q fragment
//    is q[head][64 hi + 8 s .. + 7]: each lane reads 128 contiguous bytes of
//    its head's row straight from global memory, once per kernel — Q is at
//    most 8 KiB per block and hits the cache for three of the four waves, so
//    it is not staged in LDS;
//  * scales never touch the operands: s = acc * kscale[row] * scale, and
//    p * vscale[row] goes into the bf16 pack of P (acc_to_bfrags) while the
//    row sum l keeps the unscaled p. Lane `row` loads the two scales of its
//    row (two registers to prefetch) and parks them in a per-wave LDS
//    vector; the C-register order reads them back as f32x4 broadcasts;
//  * O^T += V^T · P^T: V needs the transpose, so lane `row` loads its 128
//    bytes, converts to bf16 and writes them into a per-wave [64][128] bf16
//    PANEL tile (attention.hip); V^T A-fragments come from
//    ds_read_b64_tr_b16. The accumulators hold d on the registers and the
//    head on the lane: rescale is the lane's own scalar;
//  * the loads of the wave's next page (K 32 + V 32 + 2 registers) are
//    issued before the MFMAs of the current one. (As compiled today the
//    copy cur = nxt is scheduled right behind them, so they are also
//    WAITED for before the MFMAs and the second wave of the SIMD covers
//    the latency: docs/KERNELS.md, "FP8 paged decode".);
//  * rows >= L of the last page: V rows and both scales are staged as
//    zeros (not loaded), the score is set to -inf by an explicit select on
//    the row index (never by arithmetic: a NaN byte pattern in such a K row
//    makes its acc NaN, and NaN * 0 is NaN). A page past L is never looked
//    up; a hole in the table (entry < 0 or >= num_pages) is skipped, never
//    dereferenced. Every tile that is computed has row 0 valid, so the
//    running max is finite after it and exp() never sees -inf - -inf;
//  * the four waves merge through LDS (the V tiles, free by then, hold the
//    four [32 heads][128] fp32 partials, 16-byte slots XORed with the head so
//    the per-lane rows spread over the banks); per-split partials (o, m, l)
//    leave in the layout attn_decode_merge_kernel reads. An empty split or a
//    length of 0 writes m = -inf, l = 0, o = 0 and reads no table entry.
//
// Include AFTER attention.hip (mfma32, c_row, pack_bf2, acc_to_bfrags,
// half_pair_*, BFrag), paged.hip and decode.hip (the merge kernel).

#include "common.h"

// The kernels of this file are compiled without the packed fp32 VALU forms.
#define KV8_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__

#define KV8_WAVES 4
#define KV8_MAX_G 32                       // heads per kv head: the MFMA N
#define KV8_SLAB (PG_ROWS * PG_D)          // bytes of one (page, kv head)
#define KV8_TILE (PG_ROWS * PG_D)          // bf16 elements of a V tile

typedef __attribute__((ext_vector_type(4))) unsigned int kv8_u4;
typedef __attribute__((ext_vector_type(2))) unsigned int kv8_u2;

// ------------------------------------------------------------ quantise
// 8 fp32 -> 8 E4M3 bytes (v_cvt_pk_fp8_f32, RNE, memory order)
DEV kv8_u2 kv8_pack8(const float* f) {
  int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
  kv8_u2 out;
  out[0] = (unsigned int)w0;
  out[1] = (unsigned int)w1;
  return out;
}

// One row's share of 8 elements: amax over the 16 lanes that hold the row
// (register-file exchange), the row's scale, and the 8 bytes.
DEV kv8_u2 kv8_quant_share(bf16x8 x, float& row_scale) {
  float f[8];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] = bf2f(x[j]);
    amax = fmaxf(amax, fabsf(f[j]));
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 16));
  row_scale = __fdiv_rn(amax, 448.f);
  const float inv = amax > 0.f ? __fdiv_rn(448.f, amax) : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = fminf(fmaxf(f[j] * inv, -448.f), 448.f);
  return kv8_pack8(f);
}

// Scatter S new rows per sequence into the FP8 pool through the block
// table: the contract of kv_page_write_kernel (paged.hip). Sixteen lanes own
// one row (one bf16x8 each), K and V in one launch; lane 0 of the group
// stores the two scales. The row count times 16 is a multiple of 16 and a
// block starts on a multiple of 256, so the 16 lanes of a row are inside
// the bounds or outside them together; the reduction runs unconditionally
// (dropped rows reduce zeros).
KV8_KERNEL void __launch_bounds__(256) kv_page_write_fp8_kernel(
    const short* __restrict__ k, const short* __restrict__ v,
    unsigned char* __restrict__ kp, unsigned char* __restrict__ vp,
    float* __restrict__ ksc, float* __restrict__ vsc,
    const int* __restrict__ table, const int* __restrict__ pos,
    int B, int Hkv, int S, int num_pages, int table_stride,
    long long ksb, long long ksh, long long kss,
    long long vsb, long long vsh, long long vss) {
  constexpr int V8 = PG_D / 8;  // lanes per row
  const long long total = (long long)B * Hkv * S * V8;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < total;
       i0 += stride) {
    const long long i = i0 + threadIdx.x;
    bool ok = i < total;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 kx = z, vx = z;
    long long dst_row = 0;  // row index into [num_pages * Hkv * 64]
    const int d8 = (int)(i % V8);
    if (ok) {
      long long t = i / V8;
      const int s = (int)(t % S);
      t /= S;
      const int hk = (int)(t % Hkv);
      const int b = (int)(t / Hkv);
      const int p = pos[b];
      const long long row = (long long)p + s;
      const long long pg = row / PG_ROWS;
      ok = p >= 0 && pg < table_stride;
      if (ok) {
        const int page = table[(long long)b * table_stride + pg];
        ok = page >= 0 && page < num_pages;
        if (ok) {
          dst_row = ((long long)page * Hkv + hk) * PG_ROWS + (row % PG_ROWS);
          kx = *(const bf16x8*)(k + b * ksb + hk * ksh + s * kss + d8 * 8);
          vx = *(const bf16x8*)(v + b * vsb + hk * vsh + s * vss + d8 * 8);
        }
      }
    }
    float k_scale, v_scale;
    const kv8_u2 kb = kv8_quant_share(kx, k_scale);
    const kv8_u2 vb = kv8_quant_share(vx, v_scale);
    if (ok) {
      *(kv8_u2*)(kp + dst_row * PG_D + d8 * 8) = kb;
      *(kv8_u2*)(vp + dst_row * PG_D + d8 * 8) = vb;
      if (d8 == 0) {
        ksc[dst_row] = k_scale;
        vsc[dst_row] = v_scale;
      }
    }
  }
}

// ------------------------------------------------------------ decode
// 4 E4M3 bytes -> 4 bf16 in memory order (exact)
DEV void kv8_cvt4(unsigned int w, unsigned int& lo, unsigned int& hi) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  lo = pack_bf2(a[0], a[1]);
  hi = pack_bf2(b[0], b[1]);
}

// 8 E4M3 bytes -> one MFMA fragment
DEV bf16x8 kv8_frag(unsigned int w0, unsigned int w1) {
  union {
    unsigned int w[4];
    bf16x8 v;
  } u;
  kv8_cvt4(w0, u.w[0], u.w[1]);
  kv8_cvt4(w1, u.w[2], u.w[3]);
  return u.v;
}

// transposed LDS read as attention.hip's tr_read, with a memory clobber:
// here the tile is rewritten by the SAME wave with no block barrier in
// between, so the compiler must not move a tile store across the read.
// Waiting (s_waitcnt lgkmcnt) is the caller's job.
DEV unsigned long long kv8_tr_read(const short* lds_ptr) {
  unsigned int addr = (unsigned int)(unsigned long long)lds_ptr;
  unsigned long long out;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(out) : "v"(addr)
               : "memory");
  return out;
}

// One page of one kv head as a wave holds it in flight: K k-permuted
// (k[t][j] = bytes 64 hi + 16 j .. + 15 of row 32 t + l32), V and the two
// scales by row (lane = row).
struct Kv8Page {
  kv8_u4 k[2][4];
  kv8_u4 v[8];
  float ks, vs;
  bool ok;  // a real pool page (wave-uniform)
};

// Issue the loads of page index u of the sequence (trow = its table row),
// or fill zeros: `want` false, a hole in the table, and for V and the
// scales every row >= L. The page goes through readfirstlane, so the
// bases are scalar.
DEV void kv8_load_page(Kv8Page& pg, bool want, const int* trow, int u,
                       int L, int num_pages, int Hkv, int hk,
                       const unsigned char* __restrict__ kp,
                       const unsigned char* __restrict__ vp,
                       const float* __restrict__ ksc,
                       const float* __restrict__ vsc, int lane, int l32,
                       int hi) {
  const kv8_u4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) pg.k[t][j] = z;
#pragma unroll
  for (int c = 0; c < 8; ++c) pg.v[c] = z;
  pg.ks = 0.f;
  pg.vs = 0.f;
  pg.ok = false;
  if (!want) return;
  const int page = __builtin_amdgcn_readfirstlane(trow[u]);
  if (page < 0 || page >= num_pages) return;
  pg.ok = true;
  const long long slab = (long long)page * Hkv + hk;
  const unsigned char* kb = kp + slab * KV8_SLAB;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pg.k[t][j] =
          *(const kv8_u4*)(kb + (t * 32 + l32) * PG_D + hi * 64 + j * 16);
  if (u * PG_ROWS + lane < L) {
    const unsigned char* vb = vp + slab * KV8_SLAB + lane * PG_D;
#pragma unroll
    for (int c = 0; c < 8; ++c) pg.v[c] = *(const kv8_u4*)(vb + c * 16);
    pg.ks = ksc[slab * PG_ROWS + lane];
    pg.vs = vsc[slab * PG_ROWS + lane];
  }
}

// q [B,H,1,128] bf16; pools [num_pages,Hkv,64,128] E4M3 bytes; scales
// [num_pages,Hkv,64] fp32; table int32 [B,table_stride]; lengths int32 [B].
// Partial per (split, b, h): o [splits,B,H,128] fp32, ml [splits,B,H,2].
KV8_KERNEL void __launch_bounds__(KV8_WAVES * WAVE)
__attribute__((amdgpu_waves_per_eu(2, 2))) attn_decode_paged_fp8_partial_kernel(
    const short* __restrict__ q, const unsigned char* __restrict__ kp,
    const unsigned char* __restrict__ vp, const float* __restrict__ ksc,
    const float* __restrict__ vsc, const int* __restrict__ table,
    const int* __restrict__ lengths, float* __restrict__ o_part,
    float* __restrict__ ml_part, int B, int H, int Hkv, int num_pages,
    int table_stride, int splits, float scale) {
  // per-wave V tile, bf16 panel layout; afterwards the fp32 merge buffer
  __shared__ __attribute__((aligned(16))) short v_s[KV8_WAVES][KV8_TILE];
  // per-wave row scales (k, v); afterwards the waves' (m, l) per head
  __shared__ __attribute__((aligned(16))) float sc_s[KV8_WAVES][2][PG_ROWS];

  const int sp = blockIdx.x;
  const int hk = blockIdx.y;
  const int b = blockIdx.z;
  const int G = H / Hkv;
  const WaveCoord c = wave_coord();
  const int wid = __builtin_amdgcn_readfirstlane(c.wid);
  const int lane = c.lane, l32 = c.l32, hi = c.hi;

  // a length can never exceed what the table row addresses
  const int L = min(lengths[b], table_stride * PG_ROWS);
  const int n_pages = (L + PG_ROWS - 1) / PG_ROWS;  // <= 0 when L <= 0
  const int chunk = (n_pages + splits - 1) / splits;
  const int u0 = sp * chunk;
  const int u1 = min(n_pages, u0 + chunk);
  const int* trow = table + (long long)b * table_stride;

  // this lane's head (clamped: always a real one), its row in registers in
  // the k order of the K fragments
  const int h = hk * G + min(l32, G - 1);
  bf16x8 q_reg[8];
  {
    const short* qrow = q + ((long long)b * H + h) * PG_D + hi * 64;
#pragma unroll
    for (int s = 0; s < 8; ++s) q_reg[s] = *(const bf16x8*)(qrow + s * 8);
  }

  float m_run = -INFINITY;
  float l_run = 0.f;
  f16f acc_o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_o[n] = (f16f){};

  short* vt = &v_s[wid][0];
  float* kst = &sc_s[wid][0][0];
  float* vst = &sc_s[wid][1][0];

  Kv8Page cur, nxt;
  kv8_load_page(cur, u0 + wid < u1, trow, u0 + wid, L, num_pages, Hkv, hk,
                kp, vp, ksc, vsc, lane, l32, hi);
  for (int u = u0 + wid; u < u1; u += KV8_WAVES) {
    // ---- V (bf16) and the row scales of this page -> the wave's LDS ----
    if (cur.ok) {
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) {
        short* dst = vt + cc * (PG_ROWS * 16) + lane * 16;
        *(bf16x8*)dst = kv8_frag(cur.v[cc][0], cur.v[cc][1]);
        *(bf16x8*)(dst + 8) = kv8_frag(cur.v[cc][2], cur.v[cc][3]);
      }
      kst[lane] = cur.ks * scale;
      vst[lane] = cur.vs;
    }
    lds_wave_fence();

    // ---- the wave's next page: loads in flight under the MFMAs ----
    kv8_load_page(nxt, u + KV8_WAVES < u1, trow, u + KV8_WAVES, L,
                  num_pages, Hkv, hk, kp, vp, ksc, vsc, lane, l32, hi);
    __builtin_amdgcn_sched_barrier(0);

    if (cur.ok) {
      // ---- S^T = K (64 x 128) @ Q^T: two 32-row halves ----
      f16f st[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        st[t] = (f16f){};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const kv8_u4 w = cur.k[t][s >> 1];
          const bf16x8 kf = (s & 1) ? kv8_frag(w[2], w[3])
                                    : kv8_frag(w[0], w[1]);
          st[t] = mfma32(kf, q_reg[s], st[t]);
        }
      }

      // ---- row scale, length mask, in-register online softmax ----
      // lane's value (t, r) is S[head][row = t*32 + c_row(r, hi)]
      const int nvalid = L - u * PG_ROWS;  // >= 1: u < n_pages
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 kq = *(const f32x4*)(kst + t * 32 + 8 * g + 4 * hi);
#pragma unroll
          for (int i = 0; i < 4; ++i) st[t][4 * g + i] *= kq[i];
        }
      if (nvalid < PG_ROWS) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (t * 32 + c_row(r, hi) >= nvalid) st[t][r] = -INFINITY;
      }
      float pmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) pmax = fmaxf(pmax, st[t][r]);
      pmax = half_pair_max(pmax);
      const float newm = fmaxf(m_run, pmax);  // finite: row 0 is valid
      const float rescale = __expf(m_run - newm);
      m_run = newm;

      // p, its unscaled row sum, and p * vscale[row] for the product
      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 vq = *(const f32x4*)(vst + t * 32 + 8 * g + 4 * hi);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float e = __expf(st[t][4 * g + i] - newm);
            psum += e;
            st[t][4 * g + i] = e * vq[i];
          }
        }
      psum = half_pair_sum(psum);
      l_run = l_run * rescale + psum;

#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[n][r] *= rescale;

      bf16x8 pb[4];
      acc_to_bfrags(st[0], pb);
      acc_to_bfrags(st[1], pb + 2);

      // ---- O^T (128 d x 32 heads) += V^T (128 x 64) @ P^T (64 x 32) ----
      // the addressing of tr_load_bfrags<64> (attention.hip)
      const int tr_off = ((lane >> 4) & 1) * (PG_ROWS * 16)
                         + (hi * 8 + ((lane >> 2) & 3)) * 16 + (lane & 3) * 4;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        BFrag bfr[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const short* src =
              vt + n * 2 * (PG_ROWS * 16) + ks * 16 * 16 + tr_off;
          bfr[n].u[0] = kv8_tr_read(src);
          bfr[n].u[1] = kv8_tr_read(src + 4 * 16);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_o[n] = mfma32(bfr[n].v, pb[ks], acc_o[n]);
      }
    }
    lds_wave_fence();
    cur = nxt;
  }

  // ---- merge the 4 waves through LDS ----
  // wave w's partial O [32 heads][128 d] fp32 goes into ITS OWN tile (the
  // same 16 KiB), 16-byte slot (d >> 2) ^ head; (m, l) per head into its
  // scale vectors
  float* red = (float*)vt;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 w;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = acc_o[n][4 * g + i];
      const int slot = (n * 8 + 2 * g + hi) ^ l32;
      *(f32x4*)(red + l32 * PG_D + slot * 4) = w;
    }
  if (hi == 0) {
    kst[l32] = m_run;
    vst[l32] = l_run;
  }
  __syncthreads();

  // thread -> (head, 16-byte slot): 32 consecutive lanes read one row.
  // Empty splits and length-0 sequences write m = -inf, l = 0, o = 0.
#pragma unroll
  for (int it = 0; it < KV8_MAX_G * 32 / (KV8_WAVES * WAVE); ++it) {
    const int idx = it * (KV8_WAVES * WAVE) + threadIdx.x;
    const int head = idx >> 5, slot = idx & 31;
    if (head >= G) continue;
    float m_blk = -INFINITY;
#pragma unroll
    for (int w = 0; w < KV8_WAVES; ++w)
      m_blk = fmaxf(m_blk, sc_s[w][0][head]);
    float l_blk = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < KV8_WAVES; ++w) {
      const float m_w = sc_s[w][0][head];
      const float f = (m_w == -INFINITY) ? 0.f : __expf(m_w - m_blk);
      l_blk += f * sc_s[w][1][head];
      const f32x4 ow = *(const f32x4*)((const float*)&v_s[w][0]
                                       + head * PG_D + (slot ^ head) * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] += f * ow[i];
    }
    const long long ph = ((long long)sp * B + b) * H + hk * G + head;
    *(f32x4*)(o_part + ph * PG_D + slot * 4) = o;
    if (slot == 0) {
      ml_part[ph * 2] = m_blk;
      ml_part[ph * 2 + 1] = l_blk;
    }
  }
}
