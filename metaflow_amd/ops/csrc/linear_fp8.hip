// Weight-only FP8 (W8A16) dense projections for gfx950: the skinny stream
// GEMM of the decode step and its helpers.
//
//   lin_stream_*_kernel  y[M, N] = x[M, K] W^T, M small, W bf16 or E4M3 bytes
//                        with one fp32 scale per row; with SWIGLU W is the
//                        packed gate|up [2 inter, K] and y = silu(g) * u
//   lin_reduce_kernel    sums the split-K partials, optional SwiGLU, rounds
//   lin_dequant_kernel   bf16[r, :] = e4m3(byte[r, :]) * scale[r]
//
// The stream is moe.hip's (k-permuted 64-byte lane loads straight into the
// MFMA A registers, two register sets, x chunks through the lds_img::off_b
// image one chunk ahead, scales on the accumulators) and its helpers are
// used as they are: moe_lane, moe_load_w, moe8_frag, moe_scales. What
// differs:
//
// Tokens per pass. A wave owns 32 weight rows and NB blocks of 32 token rows
// (NB = 1 or 2): every weight fragment, converted once, feeds NB MFMAs, so
// M <= 64 reads the weights once. The x image is [32 NB rows][128 k], two
// buffers: 16 KiB at NB = 1, 32 KiB at NB = 2; row 32 t + l32 has the XOR
// key of row l32 (the key takes the row's low four bits), so block t's
// fragment is the same lane address + 8192 t, and a thread stages rows
// tid / 16 + 16 i, i < 2 NB, at its one image offset + 4096 i. M > 64 runs
// in groups of 64 that stream the weights again: correct for any M, tuned
// for one group. Rows past M load a clamped row and store nothing.
//
// Split of K. grid (N / 128, splits): split s takes chunks [s NC / splits,
// (s + 1) NC / splits). One split finishes in the kernel (scale, SwiGLU,
// one rounding to bf16); more store scaled fp32 partials [splits, M, NW]
// (NW = N, or 2 inter: gate at column r, up at inter + r) and
// lin_reduce_kernel sums them in ascending split order. No atomics.
//
// SWIGLU. A wave streams rows r and inter + r together (NMAT = 2), so gate
// and up of one (row, token) end in the same lane and register.
//
// Included after moe.hip.

#include "common.h"
#include "attn_lds_image.h"

// rows + 16 of the staging walk: same key, 16 rows of 256 bytes further
static_assert(lds_img::off_b(16, 0) == 4096 && lds_img::off_b(32, 5) ==
              lds_img::off_b(0, 5) + 8192, "x image: key period of 16 rows");

// One chunk, as moe_chunk: issue the loads of chunk `nxt` (x pieces first,
// then the weights into wn), run the chunk in wc against LDS buffer `buf`,
// publish the x pieces in the other buffer.
template <int NMAT, int NB, typename W>
DEV void lin_chunk(const bf16x8 (&wc)[NMAT][MoeW<W>::NV],
                   bf16x8 (&wn)[NMAT][MoeW<W>::NV],
                   const W* const (&wrow)[NMAT],
                   const short* const (&xr)[2 * NB], int nxt, int buf,
                   char* lds, const MoeLane& L, f16f (&acc)[NB][NMAT]) {
  const long long kn = (long long)nxt * MOE_KC;
  bf16x8 xs[2 * NB];
#pragma unroll
  for (int i = 0; i < 2 * NB; ++i)
    xs[i] = *(const bf16x8*)(xr[i] + kn + L.xcol);
  moe_load_w<NMAT, W>(wn, wrow, kn, L);
  __builtin_amdgcn_sched_barrier(0);

  const char* xb = L.xrow + buf * (NB * MOE_XBYTES);
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    const int piece = MoeW<W>::is8 ? 8 * L.hi + f
                                   : 8 * (f >> 2) + 4 * L.hi + (f & 3);
    bf16x8 b[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t)
      b[t] = *(const bf16x8*)(xb + MOE_XBYTES * t + 16 * (piece ^ L.key));
#pragma unroll
    for (int m = 0; m < NMAT; ++m) {
      bf16x8 a;
      if constexpr (MoeW<W>::is8)
        a = moe8_frag(wc[m][f >> 1], f & 1);
      else
        a = wc[m][f];
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[t][m] = mfma32(a, b[t], acc[t][m]);
    }
  }
  char* nb = lds + (buf ^ 1) * (NB * MOE_XBYTES);
#pragma unroll
  for (int i = 0; i < 2 * NB; ++i) *(bf16x8*)(nb + L.st0 + 4096 * i) = xs[i];
  __syncthreads();
}

// acc[t][m] += W_m[lane's row, chunks c0 .. c1) * X[32 t .. 32 t + 31]^T.
// xr[i] is row tid / 16 + 16 i of the group, already clamped. All threads
// of the block call it with the same c0 < c1. The last chunk prefetches
// itself, as in moe_stream.
template <int NMAT, int NB, typename W>
DEV void lin_stream(const W* const (&wrow)[NMAT],
                    const short* const (&xr)[2 * NB], int c0, int c1,
                    char* lds, const MoeLane& L, f16f (&acc)[NB][NMAT]) {
  if (c0 >= c1) return;
  bf16x8 wa[NMAT][MoeW<W>::NV], wb[NMAT][MoeW<W>::NV];
  {
    const long long k0 = (long long)c0 * MOE_KC;
    bf16x8 xs[2 * NB];
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i)
      xs[i] = *(const bf16x8*)(xr[i] + k0 + L.xcol);
    moe_load_w<NMAT, W>(wa, wrow, k0, L);
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i)
      *(bf16x8*)(lds + L.st0 + 4096 * i) = xs[i];
  }
  __syncthreads();
  for (int ch = c0; ch < c1; ch += 2) {
    lin_chunk<NMAT, NB, W>(wa, wb, wrow, xr, min(ch + 1, c1 - 1), 0, lds, L,
                           acc);
    if (ch + 1 < c1)
      lin_chunk<NMAT, NB, W>(wb, wa, wrow, xr, min(ch + 2, c1 - 1), 1, lds, L,
                             acc);
  }
}

// x [M, K] bf16; w [NW, K] (NW = N, SWIGLU: 2 N, gate rows then up rows);
// scale fp32 [NW] (E4M3 only); y [M, N] bf16 (gridDim.y == 1) or part
// [gridDim.y, M, NW] fp32. grid (N / 128, splits).
// w is deliberately not __restrict__: as a noalias read-only argument its
// loads may cross the barrier, and the compiler sinks those of the second
// register set into the conditional second chunk, right in front of the
// MFMAs that use them (seen in the ISA: 4 loads before chunk c, 12 before
// chunk c + 1, vmcnt waits on weights just issued).
template <typename W, int NB, bool SWIGLU>
DEV void lin_stream_body(const short* __restrict__ x,
                         const W* w,
                         const float* __restrict__ scale,
                         short* __restrict__ y, float* __restrict__ part,
                         int M, int K, int N, char* lds) {
  constexpr int NMAT = SWIGLU ? 2 : 1;
  const WaveCoord c = wave_coord();
  const MoeLane L = moe_lane<W>(lds);
  const int base = blockIdx.x * MOE_ROWS + c.wid * 32;
  const int NW = NMAT * N;
  const W* wrow[NMAT];
  f32x4 s[NMAT][4];
#pragma unroll
  for (int m = 0; m < NMAT; ++m) {
    wrow[m] = w + (long long)(m * N + base + c.l32) * K;
    if constexpr (MoeW<W>::is8)
      moe_scales(reinterpret_cast<long long>(scale), m * N + base, c.hi,
                 s[m]);
  }
  const int nc = K / MOE_KC;
  const int c0 = (int)((long long)blockIdx.y * nc / gridDim.y);
  const int c1 = (int)((long long)(blockIdx.y + 1) * nc / gridDim.y);
  const int srow = threadIdx.x >> 4;

  for (int g0 = 0; g0 < M; g0 += 32 * NB) {
    const short* xr[2 * NB];
#pragma unroll
    for (int i = 0; i < 2 * NB; ++i)
      xr[i] = x + (long long)min(g0 + srow + 16 * i, M - 1) * K;
    f16f acc[NB][NMAT];
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
      for (int m = 0; m < NMAT; ++m) acc[t][m] = moe_zero();
    lin_stream<NMAT, NB, W>(wrow, xr, c0, c1, lds, L, acc);

#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int tok = g0 + 32 * t + c.l32;
      if (tok >= M) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v[NMAT];
#pragma unroll
        for (int m = 0; m < NMAT; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[m][i] = acc[t][m][4 * q + i];
            if constexpr (MoeW<W>::is8) v[m][i] *= s[m][q][i];
          }
        const int col = base + c_row(4 * q, c.hi);
        if (gridDim.y == 1) {
          f32x4 o = v[0];
          if constexpr (SWIGLU) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              o[i] = v[0][i] / (1.f + expf(-v[0][i])) * v[1][i];
          }
          uint2 pk;
          pk.x = pack_bf2(o[0], o[1]);
          pk.y = pack_bf2(o[2], o[3]);
          *(uint2*)(y + (long long)tok * N + col) = pk;
        } else {
          float* pp = part + ((long long)blockIdx.y * M + tok) * NW + col;
#pragma unroll
          for (int m = 0; m < NMAT; ++m) *(f32x4*)(pp + m * N) = v[m];
        }
      }
    }
  }
}

#define LIN_STREAM_KERNEL(name, W, NB, SW)                                   \
  MOE_KERNEL void __launch_bounds__(MOE_BLOCK)                               \
  name(const short* __restrict__ x, const W* w,                              \
       const float* __restrict__ scale, short* __restrict__ y,               \
       float* __restrict__ part, int M, int K, int N) {                      \
    __shared__ __attribute__((aligned(16))) char lds[2 * NB * MOE_XBYTES];   \
    lin_stream_body<W, NB, SW>(x, w, scale, y, part, M, K, N, lds);          \
  }

LIN_STREAM_KERNEL(lin_stream_bf16_nb1_kernel, short, 1, false)
LIN_STREAM_KERNEL(lin_stream_bf16_nb2_kernel, short, 2, false)
LIN_STREAM_KERNEL(lin_stream_bf16_nb1_swiglu_kernel, short, 1, true)
LIN_STREAM_KERNEL(lin_stream_bf16_nb2_swiglu_kernel, short, 2, true)
LIN_STREAM_KERNEL(lin_stream_fp8_nb1_kernel, moe_e4m3, 1, false)
LIN_STREAM_KERNEL(lin_stream_fp8_nb2_kernel, moe_e4m3, 2, false)
LIN_STREAM_KERNEL(lin_stream_fp8_nb1_swiglu_kernel, moe_e4m3, 1, true)
LIN_STREAM_KERNEL(lin_stream_fp8_nb2_swiglu_kernel, moe_e4m3, 2, true)

// ----------------------------------------------------------------- reduce
// y[m, col] = sum_split part[split, m, col], ascending, one rounding; with
// swiglu part is [splits, M, 2 N] and y = silu(sum gate) * (sum up). One
// thread per four columns; grid ceil(M N / 1024).
MOE_KERNEL void __launch_bounds__(256)
lin_reduce_kernel(const float* __restrict__ part, short* __restrict__ y,
                  int splits, int M, int N, int swiglu) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int nq = N / 4;
  if (idx >= (long long)M * nq) return;
  const long long m = idx / nq;
  const int col = 4 * (int)(idx % nq);
  const int NW = swiglu ? 2 * N : N;
  const long long stride = (long long)M * NW;
  const float* p = part + m * NW + col;
  f32x4 g = *(const f32x4*)p;
  for (int sp = 1; sp < splits; ++sp) {
    const f32x4 v = *(const f32x4*)(p + sp * stride);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] += v[i];
  }
  if (swiglu) {
    f32x4 u = *(const f32x4*)(p + N);
    for (int sp = 1; sp < splits; ++sp) {
      const f32x4 v = *(const f32x4*)(p + N + sp * stride);
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] += v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = g[i] / (1.f + expf(-g[i])) * u[i];
  }
  uint2 pk;
  pk.x = pack_bf2(g[0], g[1]);
  pk.y = pack_bf2(g[2], g[3]);
  *(uint2*)(y + m * N + col) = pk;
}

// ---------------------------------------------------------------- dequant
// out[r, :] = e4m3(w8[r, :]) * scale[r] in fp32, rounded once to bf16. A
// lane takes 16 bytes and writes 32; K % 16 == 0; grid-stride over the
// rows * K / 16 pieces.
MOE_KERNEL void __launch_bounds__(256)
lin_dequant_kernel(const moe_e4m3* __restrict__ w8,
                   const float* __restrict__ scale, short* __restrict__ out,
                   long long rows, int K) {
  const int kv = K / 16;
  const long long total = rows * kv;
  const long long step = (long long)gridDim.x * 256;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += step) {
    const float sc = scale[idx / kv];
    union {
      bf16x8 v;
      unsigned int w[4];
    } r, o[2];
    r.v = *(const bf16x8*)(w8 + 16 * idx);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.w[i], false);
      const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)r.w[i], true);
      o[i >> 1].w[2 * (i & 1)] = pack_bf2(a[0] * sc, a[1] * sc);
      o[i >> 1].w[2 * (i & 1) + 1] = pack_bf2(b[0] * sc, b[1] * sc);
    }
    *(bf16x8*)(out + 16 * idx) = o[0].v;
    *(bf16x8*)(out + 16 * idx + 8) = o[1].v;
  }
}
