// Prefill-time MoE feed-forward for gfx950: routing for up to 65536
// entries and tiled grouped expert GEMMs. Like moe.hip, nothing here is
// read back by the host, there are no atomics, and every grid is sized
// from shapes alone, so the block is deterministic and hipGraph-capturable.
//
//   moep_topk_kernel     per block of 256 tokens: top-k experts and weights
//                        of each token (the code of moe.hip's route), the
//                        block's entry count per expert and every entry's
//                        stable rank inside (block, expert), by ballot
//   moep_scan_kernel     one wave: counts [blocks, E] -> each block's base
//                        inside an expert's run, offset [E + 1], and the
//                        tile map of the GEMMs
//   moep_scatter_kernel  order / slot from offset + block base + rank
//   moep_gateup_kernel   h[slot] = silu(x_t Wgate^T) * (x_t Wup^T)    bf16
//   moep_dn_kernel       y[slot] = h[slot] Wdown^T                    fp32
//   moep8_gateup_kernel, moep8_dn_kernel   the same over E4M3 weights
//   (moe.hip's combine kernel, with one split, ends the block)
//
// Tile map. An M tile is MOEP_TM consecutive slots of one expert. Their
// number depends on the routing, sum_e ceil(n_e / TM), but never exceeds
// entries / TM + min(E, entries): the grid has that many tiles, the scan
// kernel writes (expert, first slot) for the tiles in use and expert = -1
// for the rest, whose blocks exit at once. An expert without entries has no
// tile and costs nothing.
//
// The GEMMs. At prefill an expert sees hundreds of rows, so the weights
// have to be reused on chip. A block of 4 waves takes one M tile (128
// entries) and 128 weight rows (of Wgate and the same rows of Wup, or of
// Wdown); a wave owns 64 weight rows x 64 entries, i.e. 2 x 2 MFMA blocks
// per matrix. In the mfma32 convention (A * B^T, lane index = M/N
// coordinate) the weight rows are the A operand and the entries the B
// operand, as in moe.hip, so a lane ends up with 16 weight rows of its
// entry: gate and up of one (row, entry) share lane and register, SwiGLU is
// elementwise before the only rounding, and the stores are 4 consecutive
// elements of the entry's row. Both operands are K-contiguous rows; they
// pass through LDS in K chunks of 64 as images of [128 rows][64 k] bf16
// (16 KiB each: entries, W, and for gate/up the second W). A weight
// fragment read from LDS feeds two MFMAs, an entry fragment two per
// matrix. Two buffers: chunk c + 1 travels global -> registers while chunk
// c is multiplied, is written to the other buffer afterwards, and one
// barrier ends the chunk.
//
// The image (moep_off): 128-byte rows whose eight 16-byte pieces are XORed
// with (row >> 1) & 7. A fragment read (16 consecutive lanes = 16
// consecutive rows, one logical piece) meets two row parities x eight keys,
// a staging write (16 consecutive lanes = the 8 pieces of two consecutive
// rows) two parities x eight pieces: either way each of the sixteen
// 16-byte bank groups once. It is lds_img::off_b folded to half the row.
//
// Every (entry, weight row) product is summed over k in ascending MFMA
// steps from zero, whatever else shares the tile: a token's result does not
// depend on where the routing puts it. Entry rows past the end of the
// expert's run load a clamped row (inside x or h) and store nothing.
//
// E4M3 weights (moe.hip's format: bytes and one fp32 scale per weight row).
// A weight row's chunk is 64 bytes, four 16-byte pieces: thread tid loads
// piece tid % 4 of rows tid / 4 + 64 p, p = 0..1, of every weight image (two
// loads where bf16 has four), converts the 16 bytes to bf16 in registers
// after the chunk's MFMAs and writes them as pieces 2 (tid % 4) and + 1 of
// the same image, so fragment reads and the MFMA loop are those of bf16.
// That write: 16 consecutive lanes are 4 pieces of 4 consecutive rows, whose
// keys are a, a, a + 1, a + 1 with a even: even (or odd) pieces XORed with
// an even key stay even (odd), with an odd key turn odd (even), and the two
// rows of a key differ in parity, so the 16 lanes again meet each 16-byte
// bank group once. The scales multiply the fp32 accumulators in the
// epilogue, four f32x4 loads per 32 weight rows in C-register order.
//
// Included after moe.hip (MOE_KERNEL, moe_gvec, moe_zero, MoeW, moe8_frag,
// moe_scales, the limits).

#define MOEP_TM 128   // entries per M tile
#define MOEP_TN 128   // weight rows per block
#define MOEP_KC 64    // k elements per chunk
#define MOEP_BLOCK 256
#define MOEP_IMG (128 * MOEP_KC * 2)  // one image, bytes
#define MOEP_RT 256   // tokens per route block (one per thread)
#define MOEP_MAX_ENTRIES 65536

// ------------------------------------------------------------------ route
MOE_KERNEL void __launch_bounds__(MOEP_RT)
moep_topk_kernel(const float* __restrict__ logits, int T, int E, int k,
                 int* __restrict__ expert, float* __restrict__ weight,
                 int* __restrict__ rank, int* __restrict__ cnt) {
  __shared__ unsigned char sel[MOEP_RT * MOE_MAX_K];
  const int t0 = blockIdx.x * MOEP_RT;
  const int nt = min(MOEP_RT, T - t0), n = nt * k;

  if ((int)threadIdx.x < nt) {
    const long long t = t0 + threadIdx.x;
    const float* row = logits + t * E;
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
        sel[threadIdx.x * k + j] = (unsigned char)bi;
        expert[t * k + j] = bi;
        val[j] = best;
      }
    }
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

  // a wave walks the block's entries in index order for each of its
  // experts; the ballot ranks the matching lanes
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  int* brank = rank + (long long)t0 * k;
  for (int e = wid; e < E; e += MOEP_RT / WAVE) {
    int run = 0;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
      const int i = i0 + lane;
      const bool hit = i < n && sel[i] == e;
      const unsigned long long b = __ballot(hit);
      if (hit) brank[i] = run + __popcll(b & ((1ull << lane) - 1ull));
      run += __popcll(b);
    }
    if (lane == 0) cnt[blockIdx.x * E + e] = run;
  }
}

// cnt [nb, E]: in, a block's entries per expert; out, the entries of the
// expert in the blocks before it. tiles [max_tiles] (expert, first slot).
MOE_KERNEL void __launch_bounds__(WAVE)
moep_scan_kernel(int* __restrict__ cnt, int nb, int E, int max_tiles,
                 int* __restrict__ offset, int2* __restrict__ tiles) {
  __shared__ int tot[MOE_MAX_E];
  __shared__ int off[MOE_MAX_E + 1];
  __shared__ int tbeg[MOE_MAX_E + 1];
  const int e = threadIdx.x;
  if (e < E) {
    int acc = 0;
    for (int b = 0; b < nb; ++b) {
      const int c = cnt[b * E + e];
      cnt[b * E + e] = acc;
      acc += c;
    }
    tot[e] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0, tacc = 0;
    for (int i = 0; i < E; ++i) {
      off[i] = acc;
      offset[i] = acc;
      tbeg[i] = tacc;
      acc += tot[i];
      tacc += (tot[i] + MOEP_TM - 1) / MOEP_TM;
    }
    off[E] = acc;
    offset[E] = acc;
    tbeg[E] = tacc;
  }
  __syncthreads();
  if (e < E) {
    const int nt = tbeg[e + 1] - tbeg[e];
    for (int i = 0; i < nt; ++i)
      tiles[tbeg[e] + i] = make_int2(e, off[e] + i * MOEP_TM);
  }
  for (int i = tbeg[E] + threadIdx.x; i < max_tiles; i += WAVE)
    tiles[i] = make_int2(-1, 0);
}

// slot holds the ranks of moep_topk_kernel on entry
MOE_KERNEL void __launch_bounds__(MOEP_RT)
moep_scatter_kernel(const int* __restrict__ expert,
                    const int* __restrict__ cnt,
                    const int* __restrict__ offset, int T, int E, int k,
                    int* __restrict__ order, int* __restrict__ slot) {
  const int t0 = blockIdx.x * MOEP_RT;
  const int n = min(MOEP_RT, T - t0) * k;
  for (int i = threadIdx.x; i < n; i += MOEP_RT) {
    const int gi = t0 * k + i;
    const int e = expert[gi];
    const int p = offset[e] + cnt[blockIdx.x * E + e] + slot[gi];
    order[p] = gi;
    slot[gi] = p;
  }
}

// --------------------------------------------------------- the tile loop
DEV constexpr int moep_off(int row, int ch) {
  return 128 * row + 16 * (ch ^ ((row >> 1) & 7));
}

// The lane addressing of a block, fixed for the kernel's life. Staging:
// thread tid moves piece tid % 8 of rows tid / 8 + 32 p, p = 0..3, of every
// image; adding 32 to a row leaves its key alone, so the four image
// offsets are st + 4096 p.
struct MoepLane {
  int st;      // moep_off(tid / 8, tid % 8)
  int stw;     // weight images: st, or for E4M3 moep_off(tid / 4, 2 (tid % 4))
  int fo[4];   // fragment read, k-step s: piece (2 s + hi) ^ key of row l32
  int arow;    // byte offset of the wave's first weight row + l32
  int brow;    // and of its first entry row + l32
};

template <typename W>
DEV MoepLane moep_lane() {
  const WaveCoord c = wave_coord();
  MoepLane L;
  L.st = moep_off(threadIdx.x >> 3, threadIdx.x & 7);
  L.stw = MoeW<W>::is8 ? moep_off(threadIdx.x >> 2, 2 * (threadIdx.x & 3))
                       : L.st;
  const int key = (c.l32 >> 1) & 7;
#pragma unroll
  for (int s = 0; s < 4; ++s) L.fo[s] = 16 * ((2 * s + c.hi) ^ key);
  L.arow = 128 * (64 * (c.wid >> 1) + c.l32);
  L.brow = 128 * (64 * (c.wid & 1) + c.l32);
  return L;
}

// acc[m][i][j] += W_m[rows 64 wr + 32 i ..] * X[entries 64 we + 32 j ..]^T
// over nc chunks of K, for NMAT weight matrices that share rows and X.
// er[p]: the entry row (already clamped) this thread stages as row tid / 8
// + 32 p of the tile, at its piece; wr[m]: row tid / 8 of the block's
// weight rows at its piece, the rows + 32 p being wstep elements on (E4M3:
// row tid / 4 at its 16-byte piece, the row + 64 being wstep bytes on). The
// last chunk "prefetches" itself rather than branch: served from cache,
// never out of range.
template <int NMAT, typename W>
DEV void moep_tile(const short* const (&er)[4],
                   const W* const (&wr)[NMAT], long long wstep, int nc,
                   char* lds, const MoepLane& L,
                   f16f (&acc)[NMAT][2][2]) {
  constexpr int BUF = (1 + NMAT) * MOEP_IMG;
  constexpr int NW = MoeW<W>::is8 ? 2 : 4;  // weight loads per image
  bf16x8 se[4], sw[NMAT][NW];

  auto load = [&](int ch) {
    const long long k0 = (long long)ch * MOEP_KC;
#pragma unroll
    for (int p = 0; p < 4; ++p) se[p] = *(const bf16x8*)(er[p] + k0);
#pragma unroll
    for (int m = 0; m < NMAT; ++m)
#pragma unroll
      for (int p = 0; p < NW; ++p)
        sw[m][p] = *(moe_gvec)(wr[m] + p * wstep + k0);
  };
  auto publish = [&](int buf) {
    char* b = lds + buf * BUF + L.st;
#pragma unroll
    for (int p = 0; p < 4; ++p) *(bf16x8*)(b + 4096 * p) = se[p];
#pragma unroll
    for (int m = 0; m < NMAT; ++m)
#pragma unroll
      for (int p = 0; p < NW; ++p) {
        if constexpr (MoeW<W>::is8) {
          // pieces 2c and 2c + 1 of one row sit 16 bytes apart either way
          char* w = lds + buf * BUF + (1 + m) * MOEP_IMG + 8192 * p;
          *(bf16x8*)(w + L.stw) = moe8_frag(sw[m][p], 0);
          *(bf16x8*)(w + (L.stw ^ 16)) = moe8_frag(sw[m][p], 1);
        } else {
          *(bf16x8*)(b + (1 + m) * MOEP_IMG + 4096 * p) = sw[m][p];
        }
      }
  };

  load(0);
  publish(0);
  __syncthreads();
  for (int ch = 0; ch < nc; ++ch) {
    load(min(ch + 1, nc - 1));
    // keep the loads in front of the MFMAs (see moe_chunk)
    __builtin_amdgcn_sched_barrier(0);
    const char* xb = lds + (ch & 1) * BUF + L.brow;
    const char* wb = lds + (ch & 1) * BUF + MOEP_IMG + L.arow;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      bf16x8 b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = *(const bf16x8*)(xb + 4096 * j + L.fo[s]);
#pragma unroll
      for (int m = 0; m < NMAT; ++m)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const bf16x8 a =
              *(const bf16x8*)(wb + m * MOEP_IMG + 4096 * i + L.fo[s]);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[m][i][j] = mfma32(a, b[j], acc[m][i][j]);
        }
    }
    publish((ch + 1) & 1);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- gate/up
// x [T, hidden] bf16; tab int64 [3, E] (E4M3: [6, E], the scale addresses
// behind the weights'); h [T*k, inter] bf16 in slot order. grid (max_tiles,
// inter / 128): the M tiles of one weight tile run side by side, so an
// expert's weight rows are shared in L2 by its tiles. One body for both
// weight types under thin kernels.
template <typename W>
DEV void moep_gu_body(const short* __restrict__ x,
                      const long long* __restrict__ tab,
                      const int* __restrict__ order,
                      const int* __restrict__ offset,
                      const int2* __restrict__ tiles, short* __restrict__ h,
                      int E, int k, int hidden, int inter, char* lds) {
  constexpr bool is8 = MoeW<W>::is8;
  const int2 tl = tiles[blockIdx.x];
  if (tl.x < 0) return;
  const int e = tl.x, slot0 = tl.y, end = offset[e + 1];
  const WaveCoord c = wave_coord();
  const MoepLane L = moep_lane<W>();
  const int srow = threadIdx.x >> 3, scol = 8 * (threadIdx.x & 7);
  const int n0 = blockIdx.y * MOEP_TN;

  const short* er[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int t = order[min(slot0 + srow + 32 * p, end - 1)] / k;
    er[p] = x + (long long)t * hidden + scol;
  }
  const long long w0 =
      is8 ? (long long)(n0 + (threadIdx.x >> 2)) * hidden +
                16 * (threadIdx.x & 3)
          : (long long)(n0 + srow) * hidden + scol;
  const W* const wr[2] = {reinterpret_cast<const W*>(tab[e]) + w0,
                          reinterpret_cast<const W*>(tab[E + e]) + w0};

  f16f acc[2][2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[m][i][j] = moe_zero();
  moep_tile<2, W>(er, wr, (is8 ? 64ll : 32ll) * hidden, hidden / MOEP_KC,
                  lds, L, acc);

  f32x4 sg[2][4], su[2][4];
  if constexpr (is8) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r0 = n0 + 64 * (c.wid >> 1) + 32 * i;
      moe_scales(tab[3 * E + e], r0, c.hi, sg[i]);
      moe_scales(tab[4 * E + e], r0, c.hi, su[i]);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int s = slot0 + 64 * (c.wid & 1) + 32 * j + c.l32;
    if (s < end) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        short* hp = h + (long long)s * inter + n0 + 64 * (c.wid >> 1) +
                    32 * i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float gt = acc[0][i][j][4 * q + r], up = acc[1][i][j][4 * q + r];
            if constexpr (is8) {
              gt *= sg[i][q][r];
              up *= su[i][q][r];
            }
            v[r] = gt / (1.f + expf(-gt)) * up;
          }
          uint2 pk;
          pk.x = pack_bf2(v[0], v[1]);
          pk.y = pack_bf2(v[2], v[3]);
          *(uint2*)(hp + c_row(4 * q, c.hi)) = pk;
        }
      }
    }
  }
}

MOE_KERNEL void __launch_bounds__(MOEP_BLOCK)
moep_gateup_kernel(const short* __restrict__ x,
                   const long long* __restrict__ tab,
                   const int* __restrict__ order,
                   const int* __restrict__ offset,
                   const int2* __restrict__ tiles, short* __restrict__ h,
                   int E, int k, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 3 * MOEP_IMG];
  moep_gu_body<short>(x, tab, order, offset, tiles, h, E, k, hidden, inter,
                      lds);
}

MOE_KERNEL void __launch_bounds__(MOEP_BLOCK)
moep8_gateup_kernel(const short* __restrict__ x,
                    const long long* __restrict__ tab,
                    const int* __restrict__ order,
                    const int* __restrict__ offset,
                    const int2* __restrict__ tiles, short* __restrict__ h,
                    int E, int k, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 3 * MOEP_IMG];
  moep_gu_body<moe_e4m3>(x, tab, order, offset, tiles, h, E, k, hidden,
                         inter, lds);
}

// ------------------------------------------------------------------- down
// y [T*k, hidden] fp32 in slot order. grid (max_tiles, hidden / 128). The
// whole of inter is summed in one block: no split of K.
template <typename W>
DEV void moep_dn_body(const short* __restrict__ h,
                      const long long* __restrict__ tab,
                      const int* __restrict__ offset,
                      const int2* __restrict__ tiles, float* __restrict__ y,
                      int E, int hidden, int inter, char* lds) {
  constexpr bool is8 = MoeW<W>::is8;
  const int2 tl = tiles[blockIdx.x];
  if (tl.x < 0) return;
  const int e = tl.x, slot0 = tl.y, end = offset[e + 1];
  const WaveCoord c = wave_coord();
  const MoepLane L = moep_lane<W>();
  const int srow = threadIdx.x >> 3, scol = 8 * (threadIdx.x & 7);
  const int n0 = blockIdx.y * MOEP_TN;

  const short* er[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    er[p] = h + (long long)min(slot0 + srow + 32 * p, end - 1) * inter +
            scol;
  const long long w0 =
      is8 ? (long long)(n0 + (threadIdx.x >> 2)) * inter +
                16 * (threadIdx.x & 3)
          : (long long)(n0 + srow) * inter + scol;
  const W* const wr[1] = {reinterpret_cast<const W*>(tab[2 * E + e]) + w0};

  f16f acc[1][2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[0][i][j] = moe_zero();
  moep_tile<1, W>(er, wr, (is8 ? 64ll : 32ll) * inter, inter / MOEP_KC, lds,
                  L, acc);

  f32x4 sd[2][4];
  if constexpr (is8) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      moe_scales(tab[5 * E + e], n0 + 64 * (c.wid >> 1) + 32 * i, c.hi,
                 sd[i]);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int s = slot0 + 64 * (c.wid & 1) + 32 * j + c.l32;
    if (s < end) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float* yp = y + (long long)s * hidden + n0 + 64 * (c.wid >> 1) +
                    32 * i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[r] = acc[0][i][j][4 * q + r];
            if constexpr (is8) v[r] *= sd[i][q][r];
          }
          *(f32x4*)(yp + c_row(4 * q, c.hi)) = v;
        }
      }
    }
  }
}

MOE_KERNEL void __launch_bounds__(MOEP_BLOCK)
moep_dn_kernel(const short* __restrict__ h,
               const long long* __restrict__ tab,
               const int* __restrict__ offset,
               const int2* __restrict__ tiles, float* __restrict__ y,
               int E, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 2 * MOEP_IMG];
  moep_dn_body<short>(h, tab, offset, tiles, y, E, hidden, inter, lds);
}

MOE_KERNEL void __launch_bounds__(MOEP_BLOCK)
moep8_dn_kernel(const short* __restrict__ h,
                const long long* __restrict__ tab,
                const int* __restrict__ offset,
                const int2* __restrict__ tiles, float* __restrict__ y,
                int E, int hidden, int inter) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 2 * MOEP_IMG];
  moep_dn_body<moe_e4m3>(h, tab, offset, tiles, y, E, hidden, inter, lds);
}
