// Paged KV cache for gfx950: flash-decode that follows a block table,
// and the scatter that writes new K/V rows into the page pool.
//
// Layout (fixed, shared with models/llama.py PagedKVCache):
//  * a page is PG_ROWS = 64 cache rows — the row tile one wave owns in
//    decode.hip — so a wave tile is exactly one page: one table lookup,
//    wave-uniform;
//  * pool k_pages / v_pages: [num_pages, Hkv, 64, 128] bf16; the 64 rows
//    of one (page, kv head) are one contiguous 16 KiB run, so the
//    row-per-lane vec8 K loads coalesce exactly as in decode.hip;
//  * block table: int32 [B, table_stride]; entry [b, j] is the pool page
//    holding rows 64j .. 64j+63 of sequence b, -1 = no page. Entry j is
//    read only for j < ceil(len_b / 64).
//
// The decode kernel keeps decode.hip's structure (grid (splits, H, B),
// 4 waves, fp32 scores, online softmax per wave, V d-per-lane, LDS merge
// of the wave partials) and feeds the same attn_decode_merge_kernel.
// Split chunks are WHOLE pages, computed on the device from lengths[b],
// so every wave tile starts on a page boundary.

#include "common.h"

#define PG_ROWS 64
#define PG_D 128

// partial per (split, b, h): o [splits,B,H,128] fp32, ml [splits,B,H,2]
__global__ __launch_bounds__(256) void attn_decode_paged_partial_kernel(
    const short* __restrict__ q,        // [B, H, 1, 128]
    const short* __restrict__ kp,       // [num_pages, Hkv, 64, 128]
    const short* __restrict__ vp,
    const int* __restrict__ table,      // [B, table_stride]
    const int* __restrict__ lengths,    // [B] valid rows per sequence
    float* __restrict__ o_part, float* __restrict__ ml_part,
    int B, int H, int Hkv, int num_pages, int table_stride, int splits,
    float scale) {
  const int sp = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hk = h / (H / Hkv);
  // a length can never exceed what the table row addresses
  const int L = min(lengths[b], table_stride * PG_ROWS);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);

  __shared__ float q_s[PG_D];
  __shared__ float red_m[4], red_l[4];
  __shared__ float red_o[4][PG_D];

  // stage the query row as fp32
  if (threadIdx.x < PG_D)
    q_s[threadIdx.x] = bf2f(q[((long long)b * H + h) * PG_D
                              + threadIdx.x]);
  __syncthreads();

  // page-aligned split: chunk in pages = ceil(ceil(L/64) / splits)
  const int n_pages = (L + PG_ROWS - 1) / PG_ROWS;   // 0 when L <= 0
  const int chunk = (n_pages + splits - 1) / splits;
  const int p0 = sp * chunk;
  const int p1 = min(n_pages, p0 + chunk);
  const int* trow = table + (long long)b * table_stride;

  float m_run = -INFINITY, l_run = 0.f;
  float o_acc[2] = {0.f, 0.f};  // lane owns d = 2*lane, 2*lane+1

  for (int pg = p0 + wid; pg < p1; pg += 4) {
    // one lookup per tile, wave-uniform (scalar register)
    const int page = __builtin_amdgcn_readfirstlane(trow[pg]);
    // an unset or out-of-pool entry contributes nothing (and is never
    // dereferenced)
    if (page < 0 || page >= num_pages) continue;
    const long long kvoff =
        ((long long)page * Hkv + hk) * (PG_ROWS * PG_D);
    const int base = pg * PG_ROWS;
    const bool valid = base + lane < L;
    // score: dot(q, K[row]) — vec8 streaming loads
    float s = -INFINITY;
    if (valid) {
      const short* krow = kp + kvoff + lane * PG_D;
      float acc = 0.f;
#pragma unroll
      for (int d8 = 0; d8 < PG_D / 8; ++d8) {
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
    const int nrows = min(PG_ROWS, L - base);
    for (int r = 0; r < nrows; ++r) {
      const float pr = __shfl(p, r, WAVE);
      if (pr != 0.f) {
        const short* vrow = vp + kvoff + r * PG_D;
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
        (((long long)sp * B + b) * H + h) * PG_D;
    o_part[po + 2 * lane] = o0;
    o_part[po + 2 * lane + 1] = o1;
    if (lane == 0) {
      const long long pm = (((long long)sp * B + b) * H + h) * 2;
      ml_part[pm] = m_blk;
      ml_part[pm + 1] = l_blk;
    }
  }
}

// Scatter S new rows per sequence into the pool through the block table:
// k, v [B, Hkv, S, 128] (element strides ksb/ksh/kss, last dim dense) go
// to rows pos[b] .. pos[b]+S-1. K and V in one launch, one 16-byte vector
// per thread per tensor. pos[b] < 0 skips the sequence; a row whose table
// entry is unset or outside the pool is dropped, never written.
__global__ __launch_bounds__(256) void kv_page_write_kernel(
    const short* __restrict__ k, const short* __restrict__ v,
    short* __restrict__ kp, short* __restrict__ vp,
    const int* __restrict__ table, const int* __restrict__ pos,
    int B, int Hkv, int S, int num_pages, int table_stride,
    long long ksb, long long ksh, long long kss,
    long long vsb, long long vsh, long long vss) {
  constexpr int V8 = PG_D / 8;  // vectors per row
  const long long total = (long long)B * Hkv * S * V8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int d8 = (int)(i % V8);
    long long t = i / V8;
    const int s = (int)(t % S);
    t /= S;
    const int hk = (int)(t % Hkv);
    const int b = (int)(t / Hkv);
    const int p = pos[b];
    if (p < 0) continue;
    const long long row = (long long)p + s;
    const long long pg = row / PG_ROWS;
    if (pg >= table_stride) continue;
    const int page = table[(long long)b * table_stride + pg];
    if (page < 0 || page >= num_pages) continue;
    const long long dst =
        (((long long)page * Hkv + hk) * PG_ROWS + (row % PG_ROWS)) * PG_D
        + d8 * 8;
    *(bf16x8*)(kp + dst) =
        *(const bf16x8*)(k + b * ksb + hk * ksh + s * kss + d8 * 8);
    *(bf16x8*)(vp + dst) =
        *(const bf16x8*)(v + b * vsb + hk * vsh + s * vss + d8 * 8);
  }
}
