// Fused token sampler: [B, V] logits (bf16 or fp32, any row stride) ->
// B token ids, one workgroup per row, no sort.
//
// Per row: temperature <= 0 is greedy (argmax, lowest index among equal
// maxima). Otherwise the kept set is built from the finite entries by
// top-k (every logit >= the k-th largest, ties kept) and then top-p (the
// shortest run of distinct logit values, from the top, whose share of the
// survivors' weight reaches top_p, ties kept), and the token is the
// inverse CDF of u in vocabulary-index order over the kept weights
// w = exp((x - max) * (1/T)).
//
// Passes over the row (served from L2 after the first):
//   1. max / argmax                               -- a greedy row ends here
//   2. top-k threshold: radix descent over the order-preserving integer
//      key of the logit, one pass per 8-bit digit (bf16: 2, fp32: 4), a
//      256-bin count histogram each
//   3. top-p threshold: the same descent over weight histograms of the
//      top-k survivors; its last level also yields the kept weight W
//   4. (top-p off) one sum pass for W
//   5. block prefix sum over contiguous tiles with a running total, ended
//      at the tile in which the running weight passes u * W
// Passes 2 and 3 are skipped, block-uniformly, where the row has them off.
//
// Every sum is an integer: a weight is the fixed-point image of the fp32
// exp (w <= 1, scaled by 2^44, or less at V > 2^19 so that a row's total
// stays below 2^63), so histogram bins (LDS integer atomics), the block
// reductions and the prefix sums are exact and independent of the order
// of arrival: the result is a pure function of the inputs. Rounding enters
// only through expf and the truncation to fixed point.
//
// Histogram layout: 16 replicas per bin, replica = lane & 15, stored
// [bin][replica] as 8-byte words. The top digit of a logit row has a
// handful of populated bins; a wave whose lanes all hit one bin then adds
// to 16 distinct addresses (128 contiguous bytes, half of the 64 4-byte
// banks), four lanes each, instead of 64 lanes to one. The four-way
// same-address part remains; how the LDS serialises 64-bit atomics on it
// was not measured, and neither was another replica count.
//
// Row bases need no alignment beyond the element's: the row is read as
// 16-byte vectors from the first 16-byte boundary at or before element 0;
// the (at most two) vectors that straddle the row's ends are read element
// by element under a bounds check, so nothing outside [0, V) is touched.

#include "common.h"

#define SMP_BLOCK 1024
#define SMP_WAVES (SMP_BLOCK / WAVE)
#define SMP_BINS 256
#define SMP_REPL 16

typedef unsigned long long smp_u64;

template <typename T> struct SmpVec;
template <> struct SmpVec<short> {  // bf16
  static constexpr int VEC = 8;
  static constexpr int LEVELS = 2;
  typedef bf16x8 vec_t;
  static DEV float cvt(short v) { return bf2f(v); }
};
template <> struct SmpVec<float> {
  static constexpr int VEC = 4;
  static constexpr int LEVELS = 4;
  typedef f32x4 vec_t;
  static DEV float cvt(float v) { return v; }
};

// order-preserving key: a > b as floats <=> key(a) > key(b); -0 folded
// into +0 first so that equal logits share a key. A bf16 logit has no low
// half: clearing it (set for negatives by the complement) lets the
// descent stop after two digits.
template <typename T>
DEV unsigned int smp_key(float x) {
  x += 0.f;
  unsigned int u = __float_as_uint(x);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (SmpVec<T>::LEVELS == 2) u &= 0xffff0000u;
  return u;
}

DEV smp_u64 smp_weight(float x, float mx, float inv_t, float fix) {
  float w = expf(fminf((x - mx) * inv_t, 0.f));
  w = (w == w) ? w : 0.f;
  return (smp_u64)(w * fix);
}

// The row as 16-byte vectors: vector v holds elements s0 + v*VEC ..; s0 in
// (-VEC, 0] puts vector boundaries on 16-byte addresses.
template <typename T>
struct SmpRow {
  const T* p;
  int V, s0, nvec;

  DEV void init(const T* row, int V_) {
    constexpr int VEC = SmpVec<T>::VEC;
    p = row;
    V = V_;
    const int head =
        (int)(((16u - (unsigned)((size_t)row & 15u)) & 15u) / sizeof(T));
    s0 = head ? head - VEC : 0;
    nvec = (V - s0 + VEC - 1) / VEC;
  }

  // The raw vector v; lanes outside [0, V) are not read and hold 0.
  DEV typename SmpVec<T>::vec_t load_raw(int v) const {
    constexpr int VEC = SmpVec<T>::VEC;
    typedef typename SmpVec<T>::vec_t vec_t;
    const int i0 = s0 + v * VEC;
    if (i0 >= 0 && i0 + VEC <= V)
      return *reinterpret_cast<const vec_t*>(p + i0);
    vec_t q;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int i = i0 + j;
      q[j] = (i >= 0 && i < V) ? p[i] : (T)0;
    }
    return q;
  }

  // x[j] = element s0 + v*VEC + j of the raw vector; returns that first
  // index. The caller tests the index against [0, V).
  DEV int unpack(int v, typename SmpVec<T>::vec_t q, float* x) const {
    constexpr int VEC = SmpVec<T>::VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) x[j] = SmpVec<T>::cvt(q[j]);
    return s0 + v * VEC;
  }

  DEV int load(int v, float* x) const { return unpack(v, load_raw(v), x); }

  // f(i0, x) over every vector of the row, in no particular order, four
  // loads in flight per thread: a pass is a handful of L2 round trips per
  // thread instead of one per vector.
  template <typename F>
  DEV void for_each(F f) const {
    constexpr int VEC = SmpVec<T>::VEC;
    constexpr int U = 4;
    int v = threadIdx.x;
    for (; v + (U - 1) * SMP_BLOCK < nvec; v += U * SMP_BLOCK) {
      typename SmpVec<T>::vec_t q[U];
#pragma unroll
      for (int k = 0; k < U; ++k) q[k] = load_raw(v + k * SMP_BLOCK);
#pragma unroll
      for (int k = 0; k < U; ++k) {
        float x[VEC];
        const int i0 = unpack(v + k * SMP_BLOCK, q[k], x);
        f(i0, x);
      }
    }
    for (; v < nvec; v += SMP_BLOCK) {
      float x[VEC];
      const int i0 = load(v, x);
      f(i0, x);
    }
  }
};

DEV smp_u64 smp_shfl_up(smp_u64 v, int d) {
  unsigned int lo = __shfl_up((unsigned int)v, d, WAVE);
  unsigned int hi = __shfl_up((unsigned int)(v >> 32), d, WAVE);
  return ((smp_u64)hi << 32) | lo;
}

// inclusive scan of one value per thread over the first NT threads of the
// block (NT a multiple of 64; threads >= NT pass 0 and get garbage);
// wsum: SMP_WAVES words of LDS. Returns the inclusive prefix; *total gets
// the sum over all NT threads. Ends with a barrier.
template <int NT>
DEV smp_u64 smp_block_scan(smp_u64 v, smp_u64* wsum, smp_u64* total) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    smp_u64 t = smp_shfl_up(v, d);
    if (lane >= d) v += t;
  }
  if (lane == WAVE - 1 && wid < NT / WAVE) wsum[wid] = v;
  __syncthreads();
  smp_u64 off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / WAVE; ++w) {
    const smp_u64 s = wsum[w];
    if (w < wid) off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return v + off;
}

struct SmpShared {
  smp_u64 hist[SMP_BINS * SMP_REPL];  // 32 KiB
  smp_u64 wsum[SMP_WAVES];
  float red_val[SMP_WAVES];
  int red_idx[SMP_WAVES];
  smp_u64 sel_above, sel_incl;
  int sel_bin;
  int found, last_kept;
};

// One radix descent. WEIGHT = false: counts of all row elements, target
// `tgt` = k: the largest key t with #(key >= t) >= k. WEIGHT = true:
// weights of the elements with key >= floor_key, target the share top_p of
// their total: the largest key t whose mass(key >= t) reaches it. Returns
// t; *mass = the count or weight of key >= t.
template <typename T, bool WEIGHT>
DEV unsigned int smp_descend(const SmpRow<T>& row, SmpShared& sh, float mx,
                             float inv_t, float fix, unsigned int floor_key,
                             smp_u64 tgt, float top_p, smp_u64* mass) {
  constexpr int VEC = SmpVec<T>::VEC;
  const int tid = threadIdx.x;
  const int repl = tid & (SMP_REPL - 1);
  unsigned int prefix = 0;
  smp_u64 above = 0, incl = 0;
  for (int level = 0; level < SmpVec<T>::LEVELS; ++level) {
    const int shift = 24 - 8 * level;
    const unsigned int hi_mask = level ? (~0u << (shift + 8)) : 0u;
    for (int i = tid; i < SMP_BINS * SMP_REPL; i += SMP_BLOCK)
      sh.hist[i] = 0;
    __syncthreads();
    row.for_each([&](int i0, const float* x) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int i = i0 + j;
        const unsigned int key = smp_key<T>(x[j]);
        bool in = i >= 0 && i < row.V && ((key ^ prefix) & hi_mask) == 0;
        if (WEIGHT) in = in && key >= floor_key && x[j] > -INFINITY;
        if (in) {
          const smp_u64 add =
              WEIGHT ? smp_weight(x[j], mx, inv_t, fix) : 1ull;
          const int bin = (key >> shift) & 0xff;
          if (add) atomicAdd(&sh.hist[bin * SMP_REPL + repl], add);
        }
      }
    });
    __syncthreads();
    // thread t < 256 owns bin 255 - t: the scan runs from the top bin down
    smp_u64 own = 0;
    if (tid < SMP_BINS) {
      const smp_u64* h = &sh.hist[(SMP_BINS - 1 - tid) * SMP_REPL];
#pragma unroll
      for (int r = 0; r < SMP_REPL; ++r) own += h[r];
    }
    if (tid == 0) {
      // no crossing (a row outside the contract): the lowest bin
      sh.sel_bin = 0;
      sh.sel_above = above;
      sh.sel_incl = above;
    }
    smp_u64 total;
    smp_u64 cum = smp_block_scan<SMP_BINS>(own, sh.wsum, &total);
    if (WEIGHT && level == 0) {
      // share of the survivors' total, as an integer weight in [1, total]
      const double t = ceil((double)top_p * (double)total);
      tgt = t >= 1.0 ? (smp_u64)t : 1ull;
      if (tgt > total) tgt = total;
      if (tgt == 0) tgt = 1;
    }
    if (tid < SMP_BINS) {
      const smp_u64 c_incl = above + cum, c_excl = c_incl - own;
      if (c_incl >= tgt && c_excl < tgt) {
        sh.sel_bin = SMP_BINS - 1 - tid;
        sh.sel_above = c_excl;
        sh.sel_incl = c_incl;
      }
    }
    __syncthreads();
    prefix |= (unsigned int)sh.sel_bin << shift;
    above = sh.sel_above;
    incl = sh.sel_incl;
    __syncthreads();
  }
  *mass = incl;
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(SMP_BLOCK) void sample_tokens_kernel(
    const T* __restrict__ logits, long long row_stride, int V, float fix,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ u,
    long long* __restrict__ out) {
  constexpr int VEC = SmpVec<T>::VEC;
  __shared__ SmpShared sh;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  SmpRow<T> row;
  row.init(logits + (long long)b * row_stride, V);

  // ---- pass 1: max, and its lowest index
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  row.for_each([&](int i0, const float* x) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int i = i0 + j;
      // a thread meets its indices in rising order: > keeps the first
      // (== only takes a row's leading -inf, so an all -inf row gives 0)
      if (i >= 0 && i < V &&
          (x[j] > best || (best_i == 0x7fffffff && x[j] == best))) {
        best = x[j];
        best_i = i;
      }
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(best_i, off, WAVE);
    if (ov > best || (ov == best && oi < best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  if (lane == 0) {
    sh.red_val[wid] = best;
    sh.red_idx[wid] = best_i;
  }
  if (tid == 0) {
    sh.found = 0x7fffffff;
    sh.last_kept = -1;
  }
  __syncthreads();
  best = sh.red_val[0];
  best_i = sh.red_idx[0];
#pragma unroll
  for (int w = 1; w < SMP_WAVES; ++w) {
    const float ov = sh.red_val[w];
    const int oi = sh.red_idx[w];
    if (ov > best || (ov == best && oi < best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  // rows of NaN only: any index in range
  if (best_i < 0 || best_i >= V) best_i = 0;

  const float temp = temperature[b];
  if (!(temp > 0.f)) {
    if (tid == 0) out[b] = best_i;
    return;
  }
  const float inv_t = fminf(1.f / temp, 3.0e38f);
  const float mx = best;
  const int k = top_k[b];
  const float p = top_p[b];

  // ---- passes 2, 3: thresholds
  unsigned int thr = 0;
  smp_u64 W = 0;
  if (k > 0 && k < V) {
    smp_u64 cnt;
    thr = smp_descend<T, false>(row, sh, mx, inv_t, fix, 0u, (smp_u64)k, 0.f,
                                &cnt);
  }
  if (p < 1.f) {
    thr = smp_descend<T, true>(row, sh, mx, inv_t, fix, thr, 0ull, p, &W);
  } else {
    // ---- pass 4: the kept weight
    smp_u64 s = 0;
    row.for_each([&](int i0, const float* x) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int i = i0 + j;
        if (i >= 0 && i < V && smp_key<T>(x[j]) >= thr &&
            x[j] > -INFINITY)
          s += smp_weight(x[j], mx, inv_t, fix);
      }
    });
    smp_block_scan<SMP_BLOCK>(s, sh.wsum, &W);
  }

  // ---- pass 5: inverse CDF in index order. running > u * W with an
  // integer running weight is running > floor(u * W)
  float uu = u[b];
  uu = uu >= 0.f ? uu : 0.f;
  uu = fminf(uu, 1.f);
  const smp_u64 target = (smp_u64)((double)uu * (double)W);
  smp_u64 running = 0;
  int last = -1;
  // the next tile's vector is in flight while this tile is scanned
  typename SmpVec<T>::vec_t q_next = {};
  if (tid < row.nvec) q_next = row.load_raw(tid);
  for (int base = 0; base < row.nvec; base += SMP_BLOCK) {
    const int v = base + tid;
    const typename SmpVec<T>::vec_t q = q_next;
    if (v + SMP_BLOCK < row.nvec) q_next = row.load_raw(v + SMP_BLOCK);
    smp_u64 w[VEC];
    smp_u64 mine = 0;
    int i0 = 0;
    if (v < row.nvec) {
      float x[VEC];
      i0 = row.unpack(v, q, x);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int i = i0 + j;
        const bool keep = i >= 0 && i < V && smp_key<T>(x[j]) >= thr &&
                          x[j] > -INFINITY;
        w[j] = keep ? smp_weight(x[j], mx, inv_t, fix) : 0ull;
        mine += w[j];
        if (keep) last = i;
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) w[j] = 0;
    }
    smp_u64 tile;
    smp_u64 pre =
        running + smp_block_scan<SMP_BLOCK>(mine, sh.wsum, &tile) - mine;
    running += tile;
    if (running > target) {
      // the crossing is in this tile, at one thread's kept element
      if (pre <= target && pre + mine > target) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const smp_u64 nxt = pre + w[j];
          if (pre <= target && nxt > target) sh.found = i0 + j;
          pre = nxt;
        }
      }
      break;
    }
  }
  // rounding left no crossing (W == 0: nothing kept carries weight): the
  // last kept index, and with nothing kept the argmax
  if (last >= 0) atomicMax(&sh.last_kept, last);
  __syncthreads();
  if (tid == 0) {
    int r = sh.found;
    if (r < 0 || r >= V) r = sh.last_kept;
    if (r < 0 || r >= V) r = best_i;
    out[b] = r;
  }
}
