// Flash-decode for gfx950: one query row per (b, h) against the KV
// cache, split-K across the cache length. One kernel body,
// attn_decode_impl, serves the dense cache (attn_decode_partial_kernel)
// and the paged one (attn_decode_paged_partial_kernel).
//
// Decode is MEMORY-bound (stream L x 128 x 2 tensors of bf16 per head);
// the design maximizes streaming bandwidth and chip fill, not MFMA:
//  * grid (splits, H, B): split-K gives >> 256 workgroups even at
//    batch 1 (B*H alone cannot fill 256 CUs);
//  * 4 waves per block, each wave owns 64-row tiles of its split
//    (row-per-lane scores: lane r streams K[row r] as 16-byte vec8
//    loads — 64 consecutive rows per wave = perfectly coalesced);
//  * online softmax per wave (wave_max/wave_sum over the 64 scores),
//    V accumulated d-per-lane (lane owns 2 of the 128 columns, p_r
//    broadcast by shfl) so the [row -> column] transpose never touches
//    memory;
//  * per-wave partials merge through LDS, per-split partials (o, m, l)
//    merge in a tiny second kernel (attn_decode_merge_kernel).
//
// Dense: the cache tensors keep their FULL allocation stride (Lmax), no
// slicing copies; L marks the valid prefix, and a split is
// ceil(L / splits) rows.
// PAGED (layout in paged.hip): a wave tile is exactly one page, so its
// base comes from one block-table lookup, wave-uniform. Split chunks are
// WHOLE pages, computed on the device from lengths[b], so every wave tile
// starts on a page boundary; an unset or out-of-pool entry contributes
// nothing and is never dereferenced.
//
// Include AFTER paged.hip.

#include "common.h"

#define DEC_D 128

static_assert(DEC_D == PG_D, "head dim of the pool");
static_assert(WAVE == PG_ROWS, "one wave tile must be one page");

// The one kernel body. Dense: kc/vc [B,Hkv,Lmax,128], table null,
// num_pages and table_stride unused. PAGED: kc/vc are the pool
// [num_pages,Hkv,64,128], table int32 [B,table_stride], Lmax unused.
// Partial per (split, b, h): o [splits,B,H,128] fp32, ml [splits,B,H,2].
template <bool PAGED>
DEV void attn_decode_impl(
    const short* __restrict__ q, const short* __restrict__ kc,
    const short* __restrict__ vc, const int* __restrict__ table,
    const int* __restrict__ lengths, float* __restrict__ o_part,
    float* __restrict__ ml_part, int B, int H, int Hkv, int Lmax,
    int num_pages, int table_stride, int splits, float scale) {
  const int sp = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hk = h / (H / Hkv);
  // paged: a length can never exceed what the table row addresses
  const int L = PAGED ? min(lengths[b], table_stride * PG_ROWS) : lengths[b];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  __shared__ float q_s[DEC_D];
  __shared__ float red_m[4], red_l[4];
  __shared__ float red_o[4][DEC_D];

  // stage the query row as fp32
  if (threadIdx.x < DEC_D)
    q_s[threadIdx.x] = bf2f(q[((long long)b * H + h) * DEC_D
                              + threadIdx.x]);
  __syncthreads();

  // This split is units [u0, u1) of the sequence, a unit being one row
  // (dense) or one whole page (paged: chunk in pages =
  // ceil(ceil(L/64) / splits), 0 units when L <= 0), and rows >= row_end
  // are not valid.
  constexpr int UNIT = PAGED ? PG_ROWS : 1;
  const int n_units = (L + UNIT - 1) / UNIT;
  const int chunk = (n_units + splits - 1) / splits;
  const int u0 = sp * chunk;
  const int u1 = min(n_units, u0 + chunk);
  const int row_end = PAGED ? L : u1;
  const int* trow = PAGED ? table + (long long)b * table_stride : nullptr;

  float m_run = -INFINITY, l_run = 0.f;
  float o_acc[2] = {0.f, 0.f};  // lane owns d = 2*lane, 2*lane+1

  // a wave tile is 64 rows: WAVE / UNIT units
  for (int u = u0 + wid * (WAVE / UNIT); u < u1; u += 4 * (WAVE / UNIT)) {
    int page = 0;
    if constexpr (PAGED) {
      // one lookup per tile, wave-uniform (scalar register)
      page = __builtin_amdgcn_readfirstlane(trow[u]);
      // an unset or out-of-pool entry contributes nothing (and is never
      // dereferenced)
      if (page < 0 || page >= num_pages) continue;
    }
    // the tile's rows are [row0, row0 + 64) of the slab at kvoff: the
    // page, or the (b, kv head) slab of the dense cache
    const long long kvoff =
        PAGED ? ((long long)page * Hkv + hk) * (PG_ROWS * DEC_D)
              : ((long long)b * Hkv + hk) * Lmax * DEC_D;
    const int base = u * UNIT;
    const int row0 = PAGED ? 0 : base;
    const bool valid = base + lane < row_end;
    // score: dot(q, K[row]) — vec8 streaming loads
    float s = -INFINITY;
    if (valid) {
      const short* krow = kc + kvoff + (long long)(row0 + lane) * DEC_D;
      float acc = 0.f;
#pragma unroll
      for (int d8 = 0; d8 < DEC_D / 8; ++d8) {
        bf16x8 kv8 = *(const bf16x8*)(krow + d8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc += q_s[d8 * 8 + j] * bf2f(kv8[j]);
      }
      s = acc * scale;
    }
    const float m_new = fmaxf(m_run, wave_max(s));
    const float rescale = __expf(m_run - m_new);
    const float p = valid ? __expf(s - m_new) : 0.f;
    l_run = l_run * rescale + wave_sum(p);
    o_acc[0] *= rescale;
    o_acc[1] *= rescale;
    m_run = m_new;
    // V accumulate: lane owns 2 d-columns; p_r broadcast per row
    const int nrows = min(WAVE, row_end - base);
    for (int r = 0; r < nrows; ++r) {
      const float pr = __shfl(p, r, WAVE);
      if (pr != 0.f) {
        const short* vrow = vc + kvoff + (long long)(row0 + r) * DEC_D;
        o_acc[0] += pr * bf2f(vrow[2 * lane]);
        o_acc[1] += pr * bf2f(vrow[2 * lane + 1]);
      }
    }
  }

  // merge the 4 waves through LDS
  if (lane == 0) {
    red_m[wid] = m_run;
    red_l[wid] = l_run;
  }
  red_o[wid][2 * lane] = o_acc[0];
  red_o[wid][2 * lane + 1] = o_acc[1];
  __syncthreads();
  if (wid == 0) {
    float m_blk = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) m_blk = fmaxf(m_blk, red_m[w]);
    float l_blk = 0.f;
    float o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = (red_m[w] == -INFINITY) ? 0.f
                      : __expf(red_m[w] - m_blk);
      l_blk += f * red_l[w];
      o0 += f * red_o[w][2 * lane];
      o1 += f * red_o[w][2 * lane + 1];
    }
    // empty splits (and length-0 sequences) write m = -inf, l = 0, o = 0
    const long long po =
        (((long long)sp * B + b) * H + h) * DEC_D;
    o_part[po + 2 * lane] = o0;
    o_part[po + 2 * lane + 1] = o1;
    if (lane == 0) {
      const long long pm = (((long long)sp * B + b) * H + h) * 2;
      ml_part[pm] = m_blk;
      ml_part[pm + 1] = l_blk;
    }
  }
}

__global__ __launch_bounds__(256) void attn_decode_partial_kernel(
    const short* __restrict__ q,    // [B, H, 1, 128]
    const short* __restrict__ kc,   // [B, Hkv, Lmax, 128]
    const short* __restrict__ vc,
    const int* __restrict__ lengths,  // [B] valid prefix per sequence
    float* __restrict__ o_part, float* __restrict__ ml_part,
    int B, int H, int Hkv, int Lmax, int splits, float scale) {
  attn_decode_impl<false>(q, kc, vc, nullptr, lengths, o_part, ml_part, B, H,
                          Hkv, Lmax, 0, 0, splits, scale);
}

__global__ __launch_bounds__(256) void attn_decode_paged_partial_kernel(
    const short* __restrict__ q,        // [B, H, 1, 128]
    const short* __restrict__ kp,       // [num_pages, Hkv, 64, 128]
    const short* __restrict__ vp,
    const int* __restrict__ table,      // [B, table_stride]
    const int* __restrict__ lengths,    // [B] valid rows per sequence
    float* __restrict__ o_part, float* __restrict__ ml_part,
    int B, int H, int Hkv, int num_pages, int table_stride, int splits,
    float scale) {
  attn_decode_impl<true>(q, kp, vp, table, lengths, o_part, ml_part, B, H,
                         Hkv, 0, num_pages, table_stride, splits, scale);
}

// merge the split partials: one wave per (b, h), lane owns 2 d-columns
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(
    const float* __restrict__ o_part, const float* __restrict__ ml_part,
    short* __restrict__ o, int B, int H, int splits) {
  const int h = blockIdx.x % H;
  const int b = blockIdx.x / H;
  const int lane = threadIdx.x & (WAVE - 1);
  float m_all = -INFINITY;
  for (int sp = 0; sp < splits; ++sp)
    m_all = fmaxf(m_all,
                  ml_part[(((long long)sp * B + b) * H + h) * 2]);
  float l_all = 0.f, o0 = 0.f, o1 = 0.f;
  for (int sp = 0; sp < splits; ++sp) {
    const long long pm = (((long long)sp * B + b) * H + h) * 2;
    const float m_s = ml_part[pm];
    const float f = (m_s == -INFINITY) ? 0.f : __expf(m_s - m_all);
    l_all += f * ml_part[pm + 1];
    const long long po = (((long long)sp * B + b) * H + h) * DEC_D;
    o0 += f * o_part[po + 2 * lane];
    o1 += f * o_part[po + 2 * lane + 1];
  }
  // inactive slots (length 0) produce l_all == 0: write 0, not NaN
  const float inv = l_all > 0.f ? 1.f / l_all : 0.f;
  const long long oo = ((long long)b * H + h) * DEC_D;
  o[oo + 2 * lane] = f2bf(o0 * inv);
  o[oo + 2 * lane + 1] = f2bf(o1 * inv);
}
