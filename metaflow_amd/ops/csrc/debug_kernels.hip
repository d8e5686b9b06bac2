// Layout probe kernels: each runs one delicate lane-addressing path on
// arbitrary inputs so a host-side matmul can verify it exactly. Included
// after attention.hip in the single translation unit; the attention probe
// calls the production helpers themselves, not copies.

#include "common.h"

// probe: mfma_f32_32x32x16_bf16 layout — C = A(32x16) @ B(16x32) with
// assumed layouts: A[lane&31][(lane>>5)*8+i], B[(lane>>5)*8+i][lane&31],
// C: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5)
typedef __attribute__((ext_vector_type(16))) float f16x_;
__global__ void dbg_mfma32_kernel(const short* __restrict__ a,
                                  const short* __restrict__ b,
                                  float* __restrict__ c /* [32][32] */) {
  const int lane = threadIdx.x & 63;
  const int l32 = lane & 31;
  const int hi = lane >> 5;
  bf16x8 av, bv;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    av[i] = a[l32 * 16 + hi * 8 + i];       // A row-major [32][16]
    bv[i] = b[(hi * 8 + i) * 32 + l32];     // B row-major [16][32]
  }
  f16x_ acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
    c[row * 32 + l32] = acc[r];
  }
}

// probe: the attention kernels' LDS/register layout chain, one wave, in
// the forward's order: stage_panel -> frag8_panel A-fragments (S^T = t·x^T)
// -> col_to_afrags (C column -> A-fragments) -> tr_load_bfrags
// (hardware-transposed B-fragments of the same tile) -> store_acc_tile.
//   t [64][128] bf16, x [32][128] bf16
//   st_out [64][32] fp32  = t · x^T
//   o_out  [32][128] fp32 = bf16(x · t^T) · t
__global__ __launch_bounds__(64) void dbg_attn_layout_kernel(
    const short* __restrict__ t, const short* __restrict__ x,
    float* __restrict__ st_out, float* __restrict__ o_out) {
  constexpr int ROWS = 64;
  __shared__ short tp[ROWS * ATT_D];
  const WaveCoord c = wave_coord();

  stage_panel<ROWS, WAVE>(tp, t, ATT_D);
  __syncthreads();

  bf16x8 x_reg[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    x_reg[s] = *(const bf16x8*)(x + c.l32 * ATT_D + s * 16 + c.hi * 8);

  f16f st[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    st[u] = (f16f){};
#pragma unroll
    for (int s = 0; s < 8; ++s)
      st[u] = mfma32(frag8_panel<ROWS>(tp, u * 32 + c.l32,
                                       s * 16 + c.hi * 8),
                     x_reg[s], st[u]);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      st_out[(u * 32 + c_row(r, c.hi)) * 32 + c.l32] = st[u][r];
  }

  bf16x8 pa[4];
  col_to_afrags<2>(st, pa, c.hi);

  f16f acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = (f16f){};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    BFrag bfr[4];
    tr_load_bfrags<ROWS>(bfr, tp, ks * 16, c.lane, c.hi);
    asm volatile("s_waitcnt lgkmcnt(0)");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = mfma32(pa[ks], bfr[n].v, acc[n]);
  }
  store_acc_tile<false>(o_out, 0, 0, acc, c.l32, c.hi);
}

// probe: the train kernels' dual-use LDS image (attn_lds_image.h), one
// wave, in the forward's order and through the production helpers:
// stage_image -> img_row_frag A-fragments (S^T = t·x^T) -> acc_to_bfrags
// (C tile -> B-fragments, natural k order) -> img_tr_load (hardware-
// transposed A-fragments of the same tile): O^T = t^T · bf16(S^T).
//   t [64][128] bf16, x [32][128] bf16
//   st_out [64][32] fp32  = t · x^T
//   o_out  [32][128] fp32 = bf16(x · t^T) · t
__global__ __launch_bounds__(64) void dbg_attn_image_kernel(
    const short* __restrict__ t, const short* __restrict__ x,
    float* __restrict__ st_out, float* __restrict__ o_out) {
  constexpr int ROWS = 64;
  __shared__ short tp[ROWS * ATT_D];
  const WaveCoord c = wave_coord();

  stage_image<ROWS, WAVE>(tp, t, ATT_D);
  __syncthreads();

  bf16x8 x_reg[8];
#pragma unroll
  for (int s = 0; s < 8; ++s)
    x_reg[s] = *(const bf16x8*)(x + c.l32 * ATT_D + s * 16 + c.hi * 8);

  const int rb0 = lds_img::row_base_a(c.lane, 0);
  const int rb1 = lds_img::row_base_a(c.lane, 1);
  f16f st[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    st[u] = (f16f){};
#pragma unroll
    for (int s = 0; s < 8; ++s)
      st[u] = mfma32(img_row_frag(tp, rb0, rb1, u, s), x_reg[s], st[u]);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      st_out[(u * 32 + c_row(r, c.hi)) * 32 + c.l32] = st[u][r];
  }

  bf16x8 pb[4];
  acc_to_bfrags(st[0], pb);
  acc_to_bfrags(st[1], pb + 2);

  const unsigned int tb0 = lds_addr(tp) + lds_img::tr_base_a(c.lane, 0);
  const unsigned int tb1 = lds_addr(tp) + lds_img::tr_base_a(c.lane, 1);
  f16f acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = (f16f){};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    BFrag bfr[4];
    img_tr_load(bfr, tb0, tb1, ks);
    asm volatile("s_waitcnt lgkmcnt(0)");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = mfma32(bfr[n].v, pb[ks], acc[n]);
  }
  // acc[n][r] = O^T[d = n*32 + c_row(r, hi)][row = l32]
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      o_out[c.l32 * ATT_D + n * 32 + c_row(r, c.hi)] = acc[n][r];
}
