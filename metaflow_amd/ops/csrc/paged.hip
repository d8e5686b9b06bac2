// Paged KV cache for gfx950: the pool layout, and the scatter that writes
// new K/V rows into the page pool. The kernels that READ the pool are the
// PAGED instantiations of decode.hip (one query row) and append.hip (Sq
// query rows), which are included after this file.
//
// Layout (fixed, shared with models/llama.py PagedKVCache):
//  * a page is PG_ROWS = 64 cache rows — the row tile one wave owns in
//    decode.hip and the K/V tile of append.hip — so a tile is exactly one
//    page: one table lookup, uniform;
//  * pool k_pages / v_pages: [num_pages, Hkv, 64, 128] bf16; the 64 rows
//    of one (page, kv head) are one contiguous 16 KiB run, so the
//    row-per-lane vec8 K loads of decode coalesce exactly as on the dense
//    cache;
//  * block table: int32 [B, table_stride]; entry [b, j] is the pool page
//    holding rows 64j .. 64j+63 of sequence b, -1 = no page. Entry j is
//    read only for j < ceil(len_b / 64).

#include "common.h"

#define PG_ROWS 64
#define PG_D 128

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
