// Decode-time MoE feed-forward for gfx950: device routing and grouped
// expert FFN kernels. Nothing here is read back by the host, so the whole
// block is hipGraph-capturable.
//
//   moe_route_kernel    logits [T, E] fp32 -> top-k experts and weights per
//                       token, the entries (t*k + j) grouped by expert
//                       (order, offset) and each entry's slot in that order
//   moe_gate_up_kernel  h[slot] = silu(x_t Wgate^T) * (x_t Wup^T)   bf16
//   moe_down_kernel     y[split, slot] = h[slot, kpart] Wdown[:, kpart]^T
//   moe8_gate_up_kernel, moe8_down_kernel   the same over E4M3 weights
//   moe_combine_kernel  out[t] = sum_j weight[t, j] * sum_split y[.., slot]
//
// The two GEMM kernels are weight streams: at decode an expert sees a few
// tokens, so every weight element is read from HBM once, by one wave, and
// used in one MFMA. Work split: a block of 4 waves owns 128 weight rows of
// one expert (grid.x = rows / 128, grid.y = expert; the down kernel adds
// grid.z = split of the K range), a wave owns 32 of them. In the mfma32
// convention (A * B^T, lane index = M/N coordinate, attention.hip) the
// weight rows are the A operand and up to 32 routed tokens the B operand,
// so C holds weight row x token and a lane ends up with 16 rows of its
// token: gate and up of one (row, token) sit in the same lane and
// register, and SwiGLU is elementwise before the only rounding.
//
// k-permuted weight loads. The 16 products of one MFMA may be taken in any
// k order as long as A and B agree. The standard order would have a lane
// read 16 bytes of its row per MFMA, the two half-waves 32 adjacent bytes:
// 16-byte pieces scattered over 32 rows. Here, per 128-element K chunk and
// 64-element half g of it, lane (row l32, half-wave hi) reads the 64
// contiguous bytes at k = 64g + 32hi .. +31 of its row as four 16-byte
// loads, so the two half-waves consume one whole 128-byte line of the row.
// Fragment f = 4g + j of a lane is then k = 64g + 32hi + 8j .. +7, and the
// B fragment for it is 16-byte piece 8g + 4hi + j of the token's chunk row.
// Weights go from global memory straight to the A registers, one chunk
// ahead of the MFMAs that use them; they never pass through LDS.
//
// x chunks. The block's waves share the routed rows: [32 tokens][128 k]
// bf16, gathered by token index (gate/up) or read in slot order (down),
// staged through registers into LDS one chunk ahead (two 8 KiB buffers,
// one barrier per chunk). The image is lds_img::off_b (attn_lds_image.h):
// 256-byte rows whose 16-byte pieces are XORed with a key of the row that
// takes all 16 values over 16 consecutive rows, so the fragment read (16
// consecutive lanes = 16 consecutive rows, one logical piece) and the
// staging write (16 consecutive lanes = the 16 pieces of one row) both
// cover all banks once.
//
// An expert with more than 32 entries is served in groups of 32, and each
// group streams the expert's weights again: correct for any count, tuned
// for n_e <= 32 (the decode case). Lanes past the last entry of a group
// read a clamped row and store nothing. A block whose expert received no
// entry exits at once (block-uniform test of offset[e + 1] == offset[e]).
//
// E4M3 weights (W8A16). moe8_gate_up_kernel / moe8_down_kernel are the same
// bodies over one-byte weights: w[r, :] = e4m3(byte[r, :]) * scale[r], one
// fp32 scale per weight row. A 128-element chunk of a row is then ONE
// 128-byte line: lane (row l32, half-wave hi) reads the 64 contiguous bytes
// at k = 64hi .. +63 of its row as four 16-byte loads, the two half-waves
// again a whole line. Load j holds fragments f = 2j and 2j + 1: fragment f
// is k = 64hi + 8f .. +7, and its B fragment is 16-byte piece 8hi + f of the
// token's chunk row (the same LDS image, another walk through it). A chunk
// is 4 loads and 16 raw registers per matrix, half of bf16. The bytes are
// converted in registers right before their MFMA: v_cvt_pk_f32_fp8 on each
// half word and one pack per pair (exact: every E4M3 value is a bf16
// value), 8 VALU per fragment. The scales never touch the operands: a lane
// holds 16 weight rows in the C layout (c_row), so it loads their 16 scales
// per matrix once per block and multiplies the fp32 accumulators, gate and
// up each by their own before SwiGLU, down before the partial is stored.
//
// Builds on attention.hip's helpers (mfma32, f16f, wave_coord, c_row,
// pack_bf2) and is included after it, like append.hip.

#include "common.h"
#include "attn_lds_image.h"

#define MOE_WAVES 4
#define MOE_BLOCK (MOE_WAVES * WAVE)
#define MOE_ROWS (MOE_WAVES * 32)  // weight rows per block
#define MOE_KC 128                 // k elements per chunk
#define MOE_NTOK 32                // entries per group (the MFMA N)
#define MOE_XBYTES (MOE_NTOK * MOE_KC * 2)
#define MOE_MAX_E 64
#define MOE_MAX_K 8
#define MOE_MAX_ENTRIES 2048
#define MOE_ROUTE_BLOCK 256

// The kernels of this file are compiled without the packed fp32 VALU forms.
#define MOE_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__

// ------------------------------------------------------------------ route
MOE_KERNEL void __launch_bounds__(MOE_ROUTE_BLOCK)
moe_route_kernel(const float* __restrict__ logits, int T, int E, int k,
                 int* __restrict__ expert, float* __restrict__ weight,
                 int* __restrict__ order, int* __restrict__ offset,
                 int* __restrict__ slot) {
  __shared__ unsigned char sel[MOE_MAX_ENTRIES];    // expert of an entry
  __shared__ unsigned short rank[MOE_MAX_ENTRIES];  // its rank in the expert
  __shared__ int cnt[MOE_MAX_E];
  __shared__ int off[MOE_MAX_E + 1];
  const int n = T * k;

  // top-k of a row by k passes of "largest not yet taken"; the strict
  // compare keeps the lowest index among equal logits
  for (int t = threadIdx.x; t < T; t += MOE_ROUTE_BLOCK) {
    const float* row = logits + (long long)t * E;
    unsigned long long taken = 0;
    float val[MOE_MAX_K];
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j) {
      if (j < k) {
        float best = 0.f;
        int bi = -1;
        for (int e = 0; e < E; ++e) {
          const float v = row[e];
          if (!((taken >> e) & 1ull) && (bi < 0 || v > best)) {
            best = v;
            bi = e;
          }
        }
        taken |= 1ull << bi;
        sel[t * k + j] = (unsigned char)bi;
        expert[t * k + j] = bi;
        val[j] = best;
      }
    }
    // softmax over the selected logits; val[0] is their largest
    const float mx = val[0];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j)
      if (j < k) {
        val[j] = expf(val[j] - mx);
        sum += val[j];
      }
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j)
      if (j < k) weight[t * k + j] = val[j] / sum;
  }
  __syncthreads();

  // stable grouping: a wave walks the entries in index order for each of
  // its experts; the ballot ranks the matching lanes
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  for (int e = wid; e < E; e += MOE_ROUTE_BLOCK / WAVE) {
    int run = 0;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
      const int i = i0 + lane;
      const bool hit = i < n && sel[i] == e;
      const unsigned long long b = __ballot(hit);
      if (hit)
        rank[i] = (unsigned short)(run + __popcll(b & ((1ull << lane) - 1ull)));
      run += __popcll(b);
    }
    if (lane == 0) cnt[e] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int e = 0; e < E; ++e) {
      off[e] = acc;
      offset[e] = acc;
      acc += cnt[e];
    }
    off[E] = acc;
    offset[E] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += MOE_ROUTE_BLOCK) {
    const int p = off[sel[i]] + rank[i];
    order[p] = i;
    slot[i] = p;
  }
}

// ------------------------------------------------------- the weight stream
// Weight addresses come out of an integer table, which leaves the compiler
// a generic pointer and flat loads (counted against the LDS counter too):
// read them through a global-address-space pointer.
typedef const __attribute__((address_space(1))) bf16x8* moe_gvec;
typedef const __attribute__((address_space(1))) f32x4* moe_gf4;

// The weight element: short = bf16, moe_e4m3 = one OCP E4M3 byte. A chunk
// of a row is MoeW<W>::NV 16-byte loads per lane.
typedef unsigned char moe_e4m3;
template <typename W>
struct MoeW {
  static constexpr bool is8 = sizeof(W) == 1;
  static constexpr int NV = is8 ? 4 : 8;
};

// half (0 / 1) of a 16-byte load of E4M3 -> one MFMA fragment, k ascending
DEV bf16x8 moe8_frag(bf16x8 raw, int half) {
  union {
    bf16x8 v;
    unsigned int w[4];
  } r, o;
  r.v = raw;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int w = (int)r.w[2 * half + i];
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
    const auto b = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    o.w[2 * i] = pack_bf2(a[0], a[1]);
    o.w[2 * i + 1] = pack_bf2(b[0], b[1]);
  }
  return o.v;
}

// The lane addressing of one block's stream, fixed for the kernel's life.
struct MoeLane {
  int wcol;      // the lane's 64 contiguous bytes: + 64 g + wcol (bf16,
                 // half g, elements) or + wcol (E4M3, bytes)
  int xcol;      // staging: slot tid is piece tid % 16 of row tid / 16
  int st0, st1;  // its image offset, and that of row + 16
  int hi, key;   // fragment read: piece (8g + 4hi + j) ^ key of row l32
                 // (E4M3: piece (8hi + f) ^ key)
  const char* xrow;
};

template <typename W>
DEV MoeLane moe_lane(const char* lds) {
  const WaveCoord c = wave_coord();
  MoeLane L;
  L.wcol = (MoeW<W>::is8 ? 64 : 32) * c.hi;
  L.xcol = 8 * lds_img::stage16_ch(threadIdx.x);
  L.st0 = lds_img::off_b(lds_img::stage16_row(threadIdx.x),
                         lds_img::stage16_ch(threadIdx.x));
  L.st1 = lds_img::off_b(lds_img::stage16_row(threadIdx.x) + 16,
                         lds_img::stage16_ch(threadIdx.x));
  L.hi = c.hi;
  L.key = ((c.l32 & 3) << 2) | ((c.l32 >> 2) & 3);
  L.xrow = lds + 256 * c.l32;
  return L;
}

template <int NMAT, typename W>
DEV void moe_load_w(bf16x8 (&w)[NMAT][MoeW<W>::NV],
                    const W* const (&wrow)[NMAT], long long k0,
                    const MoeLane& L) {
#pragma unroll
  for (int m = 0; m < NMAT; ++m)
#pragma unroll
    for (int f = 0; f < MoeW<W>::NV; ++f) {
      if constexpr (MoeW<W>::is8)
        w[m][f] = *(moe_gvec)(wrow[m] + k0 + L.wcol + 16 * f);
      else
        w[m][f] = *(moe_gvec)(wrow[m] + k0 + 64 * (f >> 2) + L.wcol +
                              8 * (f & 3));
    }
}

// One chunk: issue the loads of chunk `nxt` (weights into wn, the two x
// pieces into registers), run the chunk in wc against LDS buffer `buf`,
// then publish the x pieces in the other buffer. The scheduling barrier
// keeps the loads in front of the MFMAs: left alone, the compiler sinks
// them to the end of the chunk, reloads wc in place and waits for them at
// once, which leaves no load in flight while a wave computes.
template <int NMAT, typename W>
DEV void moe_chunk(const bf16x8 (&wc)[NMAT][MoeW<W>::NV],
                   bf16x8 (&wn)[NMAT][MoeW<W>::NV],
                   const W* const (&wrow)[NMAT], const short* xr0,
                   const short* xr1, int nxt, int buf, char* lds,
                   const MoeLane& L, f16f (&acc)[NMAT]) {
  const long long kn = (long long)nxt * MOE_KC;
  // x first: loads return in order, and the LDS write at the end of the
  // chunk must not have to wait for the weights behind it
  const bf16x8 x0 = *(const bf16x8*)(xr0 + kn + L.xcol);
  const bf16x8 x1 = *(const bf16x8*)(xr1 + kn + L.xcol);
  moe_load_w<NMAT, W>(wn, wrow, kn, L);
  __builtin_amdgcn_sched_barrier(0);

  const char* xb = L.xrow + buf * MOE_XBYTES;
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    const int piece = MoeW<W>::is8 ? 8 * L.hi + f
                                   : 8 * (f >> 2) + 4 * L.hi + (f & 3);
    const bf16x8 b = *(const bf16x8*)(xb + 16 * (piece ^ L.key));
#pragma unroll
    for (int m = 0; m < NMAT; ++m) {
      if constexpr (MoeW<W>::is8)
        acc[m] = mfma32(moe8_frag(wc[m][f >> 1], f & 1), b, acc[m]);
      else
        acc[m] = mfma32(wc[m][f], b, acc[m]);
    }
  }
  char* nb = lds + (buf ^ 1) * MOE_XBYTES;
  *(bf16x8*)(nb + L.st0) = x0;
  *(bf16x8*)(nb + L.st1) = x1;
  __syncthreads();
}

// acc[m] += W_m[row0 + 32 wave + l32, chunks c0 .. c1) * X[entries]^T for
// NMAT weight matrices that share the rows and the X operand. wrow[m] is
// the lane's weight row; xr0 / xr1 the two X rows this thread stages (rows
// tid / 16 and tid / 16 + 16 of the group, already clamped). All threads
// of the block call it with the same c0, c1. Two register sets take turns
// (the loop is unrolled by two), so no fragment is ever copied. The last
// chunk "prefetches" itself rather than branch: served from cache, never
// out of range.
template <int NMAT, typename W>
DEV void moe_stream(const W* const (&wrow)[NMAT], const short* xr0,
                    const short* xr1, int c0, int c1, char* lds,
                    const MoeLane& L, f16f (&acc)[NMAT]) {
  if (c0 >= c1) return;
  bf16x8 wa[NMAT][MoeW<W>::NV], wb[NMAT][MoeW<W>::NV];
  moe_load_w<NMAT, W>(wa, wrow, (long long)c0 * MOE_KC, L);
  {
    const bf16x8 x0 =
        *(const bf16x8*)(xr0 + (long long)c0 * MOE_KC + L.xcol);
    const bf16x8 x1 =
        *(const bf16x8*)(xr1 + (long long)c0 * MOE_KC + L.xcol);
    *(bf16x8*)(lds + L.st0) = x0;
    *(bf16x8*)(lds + L.st1) = x1;
  }
  __syncthreads();
  for (int ch = c0; ch < c1; ch += 2) {
    moe_chunk<NMAT, W>(wa, wb, wrow, xr0, xr1, min(ch + 1, c1 - 1), 0, lds,
                       L, acc);
    if (ch + 1 < c1)
      moe_chunk<NMAT, W>(wb, wa, wrow, xr0, xr1, min(ch + 2, c1 - 1), 1, lds,
                         L, acc);
  }
}

DEV f16f moe_zero() {
  f16f z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// The 16 scales of a lane's C rows (E4M3): rows base + c_row(r, hi) of the
// fp32 [out] vector at address `addr`, as s[r / 4][r % 4].
DEV void moe_scales(long long addr, int base, int hi, f32x4 (&s)[4]) {
  const float* p = reinterpret_cast<const float*>(addr) + base;
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = *(moe_gf4)(p + c_row(4 * q, hi));
}

// ---------------------------------------------------------------- gate/up
// x [T, hidden] bf16; tab int64 [3, E] (gate, up, down weight addresses),
// for E4M3 [6, E]: then the gate, up, down scale addresses; h [T*k, inter]
// bf16 in slot order. grid (inter / 128, E). One body for both weight
// types under thin kernels.
template <typename W>
DEV void moe_gu_body(const short* __restrict__ x,
                     const long long* __restrict__ tab,
                     const int* __restrict__ order,
                     const int* __restrict__ offset, short* __restrict__ h,
                     int E, int k, int hidden, int inter, char* lds) {
  const int e = blockIdx.y;
  const int beg = offset[e], n_e = offset[e + 1] - beg;
  if (n_e == 0) return;
  const WaveCoord c = wave_coord();
  const MoeLane L = moe_lane<W>(lds);
  const int row = blockIdx.x * MOE_ROWS + c.wid * 32 + c.l32;
  const W* const wrow[2] = {
      reinterpret_cast<const W*>(tab[e]) + (long long)row * hidden,
      reinterpret_cast<const W*>(tab[E + e]) + (long long)row * hidden};
  const int srow = threadIdx.x >> 4;
  f32x4 sg[4], su[4];
  if constexpr (MoeW<W>::is8) {
    moe_scales(tab[3 * E + e], blockIdx.x * MOE_ROWS + c.wid * 32, c.hi, sg);
    moe_scales(tab[4 * E + e], blockIdx.x * MOE_ROWS + c.wid * 32, c.hi, su);
  }

  for (int g0 = 0; g0 < n_e; g0 += MOE_NTOK) {
    // the two rows this thread stages: token of entry order[..], clamped
    const int t0 = order[beg + min(g0 + srow, n_e - 1)] / k;
    const int t1 = order[beg + min(g0 + srow + 16, n_e - 1)] / k;
    f16f acc[2] = {moe_zero(), moe_zero()};
    moe_stream<2, W>(wrow, x + (long long)t0 * hidden,
                     x + (long long)t1 * hidden, 0, hidden / MOE_KC, lds, L,
                     acc);
    if (g0 + c.l32 < n_e) {
      short* hp = h + (long long)(beg + g0 + c.l32) * inter +
                  blockIdx.x * MOE_ROWS + c.wid * 32;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float gt = acc[0][4 * q + i], up = acc[1][4 * q + i];
          if constexpr (MoeW<W>::is8) {
            gt *= sg[q][i];
            up *= su[q][i];
          }
          v[i] = gt / (1.f + expf(-gt)) * up;
        }
        uint2 pk;
        pk.x = pack_bf2(v[0], v[1]);
        pk.y = pack_bf2(v[2], v[3]);
        *(uint2*)(hp + c_row(4 * q, c.hi)) = pk;
      }
    }
  }
}

MOE_KERNEL void __launch_bounds__(MOE_BLOCK)
moe_gate_up_kernel(const short* __restrict__ x,
                   const long long* __restrict__ tab,
                   const int* __restrict__ order,
                   const int* __restrict__ offset, short* __restrict__ h,
                   int E, int k, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * MOE_XBYTES];
  moe_gu_body<short>(x, tab, order, offset, h, E, k, hidden, inter, lds);
}

MOE_KERNEL void __launch_bounds__(MOE_BLOCK)
moe8_gate_up_kernel(const short* __restrict__ x,
                    const long long* __restrict__ tab,
                    const int* __restrict__ order,
                    const int* __restrict__ offset, short* __restrict__ h,
                    int E, int k, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * MOE_XBYTES];
  moe_gu_body<moe_e4m3>(x, tab, order, offset, h, E, k, hidden, inter, lds);
}

// ------------------------------------------------------------------- down
// y [splits, T*k, hidden] fp32. grid (hidden / 128, E, splits); split s
// takes chunks [s * NC / splits, (s + 1) * NC / splits) of inter.
template <typename W>
DEV void moe_dn_body(const short* __restrict__ h,
                     const long long* __restrict__ tab,
                     const int* __restrict__ offset, float* __restrict__ y,
                     int E, int entries, int hidden, int inter, char* lds) {
  const int e = blockIdx.y;
  const int beg = offset[e], n_e = offset[e + 1] - beg;
  if (n_e == 0) return;
  const WaveCoord c = wave_coord();
  const MoeLane L = moe_lane<W>(lds);
  const int row = blockIdx.x * MOE_ROWS + c.wid * 32 + c.l32;
  const W* const wrow[1] = {
      reinterpret_cast<const W*>(tab[2 * E + e]) + (long long)row * inter};
  const int nc = inter / MOE_KC;
  const int c0 = (int)((long long)blockIdx.z * nc / gridDim.z);
  const int c1 = (int)((long long)(blockIdx.z + 1) * nc / gridDim.z);
  const int srow = threadIdx.x >> 4;
  float* ys = y + (long long)blockIdx.z * entries * hidden;
  f32x4 sd[4];
  if constexpr (MoeW<W>::is8)
    moe_scales(tab[5 * E + e], blockIdx.x * MOE_ROWS + c.wid * 32, c.hi, sd);

  for (int g0 = 0; g0 < n_e; g0 += MOE_NTOK) {
    const int s0 = beg + min(g0 + srow, n_e - 1);
    const int s1 = beg + min(g0 + srow + 16, n_e - 1);
    f16f acc[1] = {moe_zero()};
    moe_stream<1, W>(wrow, h + (long long)s0 * inter,
                     h + (long long)s1 * inter, c0, c1, lds, L, acc);
    if (g0 + c.l32 < n_e) {
      float* yp = ys + (long long)(beg + g0 + c.l32) * hidden +
                  blockIdx.x * MOE_ROWS + c.wid * 32;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[0][4 * q + i];
          if constexpr (MoeW<W>::is8) v[i] *= sd[q][i];
        }
        *(f32x4*)(yp + c_row(4 * q, c.hi)) = v;
      }
    }
  }
}

MOE_KERNEL void __launch_bounds__(MOE_BLOCK)
moe_down_kernel(const short* __restrict__ h,
                const long long* __restrict__ tab,
                const int* __restrict__ offset, float* __restrict__ y,
                int E, int entries, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * MOE_XBYTES];
  moe_dn_body<short>(h, tab, offset, y, E, entries, hidden, inter, lds);
}

MOE_KERNEL void __launch_bounds__(MOE_BLOCK)
moe8_down_kernel(const short* __restrict__ h,
                 const long long* __restrict__ tab,
                 const int* __restrict__ offset, float* __restrict__ y,
                 int E, int entries, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * MOE_XBYTES];
  moe_dn_body<moe_e4m3>(h, tab, offset, y, E, entries, hidden, inter, lds);
}

// ---------------------------------------------------------------- combine
// out[t] = sum_j weight[t, j] * (sum_split y[split, slot[t*k + j]]), j then
// split ascending, fp32, one rounding. grid (ceil(hidden / 1024), T).
MOE_KERNEL void __launch_bounds__(256)
moe_combine_kernel(const float* __restrict__ y,
                   const float* __restrict__ weight,
                   const int* __restrict__ slot, short* __restrict__ out,
                   int k, int splits, int entries, int hidden) {
  const int t = blockIdx.y;
  const int col = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (col >= hidden) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    const float w = weight[t * k + j];
    const float* yp = y + (long long)slot[t * k + j] * hidden + col;
    f32x4 s = *(const f32x4*)yp;
    for (int sp = 1; sp < splits; ++sp) {
      const f32x4 v = *(const f32x4*)(yp + (long long)sp * entries * hidden);
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] += v[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += w * s[i];
  }
  uint2 pk;
  pk.x = pack_bf2(acc[0], acc[1]);
  pk.y = pack_bf2(acc[2], acc[3]);
  *(uint2*)(out + (long long)t * hidden + col) = pk;
}
