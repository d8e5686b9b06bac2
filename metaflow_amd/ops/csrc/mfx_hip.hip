// PyTorch bindings for the metaflow_amd gfx950 kernel library (_mfx_hip).
// All tensors bf16 unless stated; shapes validated here so kernels stay lean.

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#include "elementwise.hip"
#include "adam.hip"
#include "cross_entropy.hip"
#include "attention.hip"
#include "paged.hip"
#include "decode.hip"
#include "append.hip"
#include "sampling.hip"
#include "debug_kernels.hip"

namespace {

constexpr int kBlock = 256;
// memory-bound grid cap (guide G11): 256 CUs x 8 blocks
constexpr int kGridCap = 2048;

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

inline const short* bf(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr());
}
inline short* bfm(torch::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr());
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

inline int grid_for(long long work_items) {
  long long blocks = (work_items + kBlock - 1) / kBlock;
  return (int)std::min<long long>(blocks, kGridCap);
}

// ------------------------------------------------------------- rmsnorm
std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "H must be a multiple of 8");
  const long long rows = x.numel() / H;
  auto y = torch::empty_like(x);
  auto inv = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  rmsnorm_fwd_kernel<kBlock><<<(int)rows, kBlock, 0, cur_stream()>>>(
      bf(x), nullptr, nullptr, bf(w), bfm(y), inv.data_ptr<float>(), H,
      (float)eps);
  HIP_CHECK_KERNEL();
  return {y, inv};
}

std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor x,
                                           torch::Tensor res,
                                           torch::Tensor w, double eps) {
  check_bf16(x, "x");
  check_bf16(res, "res");
  const int H = x.size(-1);
  const long long rows = x.numel() / H;
  auto s = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto inv = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  rmsnorm_fwd_kernel<kBlock><<<(int)rows, kBlock, 0, cur_stream()>>>(
      bf(x), bf(res), bfm(s), bf(w), bfm(y), inv.data_ptr<float>(), H,
      (float)eps);
  HIP_CHECK_KERNEL();
  return {s, y, inv};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor x, torch::Tensor w,
                                       torch::Tensor dy,
                                       torch::Tensor inv_rms,
                                       c10::optional<torch::Tensor> dsum) {
  check_bf16(x, "x");
  check_bf16(dy, "dy");
  const int H = x.size(-1);
  const long long rows = x.numel() / H;
  auto dx = torch::empty_like(x);
  auto dw = torch::zeros({H}, x.options().dtype(torch::kFloat32));
  int grid = (int)std::min<long long>(rows, 1024);
  size_t lds = (H + kBlock / 64) * sizeof(float);
  const short* extra = dsum.has_value() ? bf(*dsum) : nullptr;
  rmsnorm_bwd_kernel<kBlock><<<grid, kBlock, lds, cur_stream()>>>(
      bf(x), bf(w), bf(dy), extra, inv_rms.data_ptr<float>(), bfm(dx),
      dw.data_ptr<float>(), (int)rows, H);
  HIP_CHECK_KERNEL();
  return {dx, dw};
}

// ---------------------------------------------------------------- rope
torch::Tensor rope(torch::Tensor x, torch::Tensor cos_t, torch::Tensor sin_t,
                   long rows_per_pos, long seqlen, long pos0, bool backward) {
  check_bf16(x, "x");
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda(),
              "rope tables must be on the GPU (host pointers fault)");
  const int D = x.size(-1);
  const long long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  const long long total = rows * (D / 2);
  rope_kernel<<<grid_for(total), kBlock, 0, cur_stream()>>>(
      bf(x), bfm(y), cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), rows,
      D, (int)rows_per_pos, (int)seqlen, (int)pos0, backward ? -1.f : 1.f);
  HIP_CHECK_KERNEL();
  return y;
}

// ----------------------------------------------------- fused qkv rope
std::vector<torch::Tensor> rope_qkv_fwd(torch::Tensor qkv,
                                        torch::Tensor cos_t,
                                        torch::Tensor sin_t, long nq,
                                        long nkv) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda(),
              "rope tables must be on the GPU (host pointers fault)");
  const int B = qkv.size(0), S = qkv.size(1);
  const int NQ = (int)nq, NKV = (int)nkv;
  TORCH_CHECK(qkv.size(2) == (long)(NQ + 2 * NKV) * 128,
              "qkv last dim must be (nq + 2*nkv) * 128");
  auto opts = qkv.options();
  auto q = torch::empty({B, NQ, S, 128}, opts);
  auto k = torch::empty({B, NKV, S, 128}, opts);
  auto v = torch::empty({B, NKV, S, 128}, opts);
  const long long total = (long long)B * S * (NQ + 2 * NKV) * 8;
  rope_qkv_fwd_kernel<<<grid_for(total), kBlock, 0, cur_stream()>>>(
      bf(qkv), bfm(q), bfm(k), bfm(v), cos_t.data_ptr<float>(),
      sin_t.data_ptr<float>(), B, S, NQ, NKV);
  HIP_CHECK_KERNEL();
  return {q, k, v};
}

torch::Tensor rope_qkv_bwd(torch::Tensor dq, torch::Tensor dk,
                           torch::Tensor dv, torch::Tensor cos_t,
                           torch::Tensor sin_t) {
  check_bf16(dq, "dq");
  check_bf16(dk, "dk");
  check_bf16(dv, "dv");
  const int B = dq.size(0), NQ = dq.size(1), S = dq.size(2);
  const int NKV = dk.size(1);
  auto dqkv = torch::empty({B, S, (long)(NQ + 2 * NKV) * 128},
                           dq.options());
  const long long total = (long long)B * S * (NQ + 2 * NKV) * 8;
  rope_qkv_bwd_kernel<<<grid_for(total), kBlock, 0, cur_stream()>>>(
      bf(dq), bf(dk), bf(dv), bfm(dqkv), cos_t.data_ptr<float>(),
      sin_t.data_ptr<float>(), B, S, NQ, NKV);
  HIP_CHECK_KERNEL();
  return dqkv;
}

// -------------------------------------------------------------- swiglu
torch::Tensor swiglu_fwd(torch::Tensor g, torch::Tensor u) {
  check_bf16(g, "g");
  check_bf16(u, "u");
  TORCH_CHECK(g.numel() % 8 == 0);
  auto y = torch::empty_like(g);
  long long n8 = g.numel() / 8;
  swiglu_fwd_kernel<<<grid_for(n8), kBlock, 0, cur_stream()>>>(
      bf(g), bf(u), bfm(y), n8);
  HIP_CHECK_KERNEL();
  return y;
}

std::vector<torch::Tensor> swiglu_bwd(torch::Tensor g, torch::Tensor u,
                                      torch::Tensor dy) {
  auto dg = torch::empty_like(g);
  auto du = torch::empty_like(u);
  long long n8 = g.numel() / 8;
  swiglu_bwd_kernel<<<grid_for(n8), kBlock, 0, cur_stream()>>>(
      bf(g), bf(u), bf(dy), bfm(dg), bfm(du), n8);
  HIP_CHECK_KERNEL();
  return {dg, du};
}

std::vector<torch::Tensor> swiglu_gu_fwd(torch::Tensor gu) {
  check_bf16(gu, "gu");
  const int I2 = gu.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "fused swiglu needs 2I % 16 == 0");
  const int I = I2 / 2;
  const long long rows = gu.numel() / I2;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto y = torch::empty(sizes, gu.options());
  long long total = rows * (I / 8);
  swiglu_gu_fwd_kernel<<<grid_for(total), kBlock, 0, cur_stream()>>>(
      bf(gu), bfm(y), rows, I);
  HIP_CHECK_KERNEL();
  return {y};
}

torch::Tensor swiglu_gu_bwd(torch::Tensor gu, torch::Tensor dy) {
  const int I = gu.size(-1) / 2;
  const long long rows = gu.numel() / (2 * I);
  auto dgu = torch::empty_like(gu);
  long long total = rows * (I / 8);
  swiglu_gu_bwd_kernel<<<grid_for(total), kBlock, 0, cur_stream()>>>(
      bf(gu), bf(dy.contiguous()), bfm(dgu), rows, I);
  HIP_CHECK_KERNEL();
  return dgu;
}

torch::Tensor decode_tokens_u16(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kUInt8, "pass raw bytes (uint8)");
  TORCH_CHECK(x.numel() % 16 == 0,
              "token buffer must hold a multiple of 8 uint16 tokens");
  const long long n = x.numel() / 2;
  auto y = torch::empty({n}, x.options().dtype(torch::kInt64));
  decode_tokens_u16_kernel<<<grid_for(n / 8), kBlock, 0, cur_stream()>>>(
      reinterpret_cast<const unsigned short*>(x.data_ptr()),
      reinterpret_cast<long long*>(y.data_ptr<int64_t>()), n / 8);
  HIP_CHECK_KERNEL();
  return y;
}

torch::Tensor quant_e4m3(torch::Tensor x, double scale) {
  check_bf16(x, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "quant_e4m3 needs numel % 8 == 0");
  auto y = torch::empty_like(x, x.options().dtype(torch::kUInt8));
  long long n8 = x.numel() / 8;
  quant_e4m3_kernel<<<grid_for(n8), kBlock, 0, cur_stream()>>>(
      bf(x), y.data_ptr<unsigned char>(), (float)scale, n8);
  HIP_CHECK_KERNEL();
  return y;
}

torch::Tensor quant_e5m2(torch::Tensor x, double scale) {
  check_bf16(x, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "quant_e5m2 needs numel % 8 == 0");
  auto y = torch::empty_like(x, x.options().dtype(torch::kUInt8));
  long long n8 = x.numel() / 8;
  quant_e5m2_kernel<<<grid_for(n8), kBlock, 0, cur_stream()>>>(
      bf(x), y.data_ptr<unsigned char>(), (float)scale, n8);
  HIP_CHECK_KERNEL();
  return y;
}

torch::Tensor add_bf16(torch::Tensor a, torch::Tensor b) {
  check_bf16(a, "a");
  TORCH_CHECK(a.numel() % 8 == 0);
  auto y = torch::empty_like(a);
  long long n8 = a.numel() / 8;
  add_bf16_kernel<<<grid_for(n8), kBlock, 0, cur_stream()>>>(
      bf(a), bf(b), bfm(y), n8);
  HIP_CHECK_KERNEL();
  return y;
}

// ---------------------------------------------------------------- adam
void adamw(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v,
           c10::optional<torch::Tensor> master, double lr, double beta1,
           double beta2, double eps, double weight_decay, long step,
           double grad_scale) {
  const long long n = p.numel();
  float bias_c1 = 1.f / (1.f - powf((float)beta1, (float)step));
  float bias_c2 = 1.f / (1.f - powf((float)beta2, (float)step));
  if (p.scalar_type() == torch::kBFloat16) {
    TORCH_CHECK(n % 4 == 0, "bf16 adamw requires numel % 4 == 0");
    float* master_ptr =
        master.has_value() ? master->data_ptr<float>() : nullptr;
    adamw_kernel<<<grid_for(n / 4), kBlock, 0, cur_stream()>>>(
        bfm(p), bf(g), m.data_ptr<float>(), v.data_ptr<float>(), master_ptr,
        n, (float)lr, (float)beta1, (float)beta2, (float)eps,
        (float)weight_decay, bias_c1, bias_c2, (float)grad_scale);
    HIP_CHECK_KERNEL();
  } else {
    adamw_f32_kernel<<<grid_for(n), kBlock, 0, cur_stream()>>>(
        p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
        v.data_ptr<float>(), n, (float)lr, (float)beta1, (float)beta2,
        (float)eps, (float)weight_decay, bias_c1, bias_c2,
        (float)grad_scale);
    HIP_CHECK_KERNEL();
  }
}

// ------------------------------------------------------- cross entropy
std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor targets,
                                             long ignore_index) {
  check_bf16(logits, "logits");
  const int V = logits.size(-1);
  const long long N = logits.numel() / V;
  auto loss = torch::empty({N}, logits.options().dtype(torch::kFloat32));
  auto rmax = torch::empty({N}, logits.options().dtype(torch::kFloat32));
  auto rlse = torch::empty({N}, logits.options().dtype(torch::kFloat32));
  int grid = (int)std::min<long long>(N, kGridCap);
  cross_entropy_fwd_kernel<kBlock><<<grid, kBlock, 0, cur_stream()>>>(
      bf(logits), reinterpret_cast<const long long*>(targets.data_ptr<int64_t>()), loss.data_ptr<float>(),
      rmax.data_ptr<float>(), rlse.data_ptr<float>(), N, V,
      (long long)ignore_index);
  HIP_CHECK_KERNEL();
  return {loss, rlse};
}

torch::Tensor cross_entropy_bwd(torch::Tensor logits, torch::Tensor targets,
                                torch::Tensor row_lse, torch::Tensor dloss,
                                long ignore_index) {
  const int V = logits.size(-1);
  const long long N = logits.numel() / V;
  auto dlogits = torch::empty_like(logits);
  int grid = (int)std::min<long long>(N, kGridCap);
  cross_entropy_bwd_kernel<kBlock><<<grid, kBlock, 0, cur_stream()>>>(
      bf(logits), reinterpret_cast<const long long*>(targets.data_ptr<int64_t>()), row_lse.data_ptr<float>(),
      dloss.data_ptr<float>(), bfm(dlogits), N, V, (long long)ignore_index);
  HIP_CHECK_KERNEL();
  return dlogits;
}

// ----------------------------------------------------------- attention
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, double scale,
                                    bool causal) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(v, "v");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hkv = k.size(1);
  TORCH_CHECK(D == 128, "attention requires head dim 128");
  // the Python wrapper pads unaligned seqlens to the 256 boundary
  // (zero end-padding is exact for causal attention)
  TORCH_CHECK(S % 256 == 0, "attention kernel requires seqlen % 256 == 0");
  TORCH_CHECK(H % Hkv == 0, "GQA requires H % Hkv == 0");
  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, S}, q.options().dtype(torch::kFloat32));
  // v2: 8-wave 32x32 swapped-QK^T structure; one block per (q tile, h,
  // b) on a 1-D grid, the kernel maps the block id heavy tiles first
  dim3 grid((S / 256) * H * B);
  attn_fwd_v2_kernel<512><<<grid, 512, 0, cur_stream()>>>(
      bf(q), bf(k), bf(v), bfm(o), lse.data_ptr<float>(), B, H, Hkv, S,
      (float)scale, causal ? 1 : 0);
  HIP_CHECK_KERNEL();
  return {o, lse};
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o,
                                    torch::Tensor dout, torch::Tensor lse,
                                    double scale, bool causal) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(v, "v");
  check_bf16(o, "o");
  check_bf16(dout, "dout");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hkv = k.size(1);
  TORCH_CHECK(D == 128, "attention requires head dim 128");
  TORCH_CHECK(S % 256 == 0, "attention kernel requires seqlen % 256 == 0");
  TORCH_CHECK(H % Hkv == 0, "GQA requires H % Hkv == 0");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat32 &&
                  lse.is_contiguous(),
              "lse must be contiguous fp32 on GPU");
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == H &&
                  lse.size(2) == S,
              "lse must have shape [B,H,S]");
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto f32opts = q.options().dtype(torch::kFloat32);
  auto delta = torch::empty({B, H, S}, f32opts);
  // dkdv writes one fp32 partial per q head, [B,H,S,D]; the reduction
  // sums the G partials per kv head (rationale in attention.hip)
  auto dk_part = torch::empty({B, H, S, 128}, f32opts);
  auto dv_part = torch::empty({B, H, S, 128}, f32opts);
  const int icausal = causal ? 1 : 0;
  // one block per (tile, h, b) on a 1-D grid: dkdv and dq map the block
  // id heavy tiles first (block_coord in attention.hip)
  const dim3 grid((S / 256) * H * B);

  {
    const long long rows = (long long)B * H * S;
    const int rows_per_block = kBlock / 64;
    const long long blocks = (rows + rows_per_block - 1) / rows_per_block;
    attn_bwd_delta_kernel<<<(int)blocks, kBlock, 0, cur_stream()>>>(
        bf(dout), bf(o), delta.data_ptr<float>(), rows);
    HIP_CHECK_KERNEL();
  }
  {
    // dkdv: static 33280 B + the 64 KiB V image exceed the 64 KiB a
    // kernel gets without asking; dq: static 32 KiB + its second K/V
    // buffer reach it. The attribute is per device.
    static bool lds_set[64] = {};
    int dev_id = 0;
    TORCH_CHECK(hipGetDevice(&dev_id) == hipSuccess && dev_id < 64,
                "attn_bwd: hipGetDevice failed");
    if (!lds_set[dev_id]) {
      hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&attn_bwd_dkdv_v2_kernel<512>),
          hipFuncAttributeMaxDynamicSharedMemorySize, DKDV_DYN_LDS);
      if (e == hipSuccess)
        e = hipFuncSetAttribute(
            reinterpret_cast<const void*>(&attn_bwd_dq_v2_kernel<512>),
            hipFuncAttributeMaxDynamicSharedMemorySize, DQ_DYN_LDS);
      TORCH_CHECK(e == hipSuccess, "attn_bwd: cannot raise dynamic LDS: ",
                  hipGetErrorString(e));
      lds_set[dev_id] = true;
    }
  }
  attn_bwd_dkdv_v2_kernel<512><<<grid, 512, DKDV_DYN_LDS, cur_stream()>>>(
      bf(q), bf(k), bf(v), bf(dout), lse.data_ptr<float>(),
      delta.data_ptr<float>(), dk_part.data_ptr<float>(),
      dv_part.data_ptr<float>(), B, H, Hkv, S, (float)scale, icausal);
  HIP_CHECK_KERNEL();
  {
    const long long n4_kv = (long long)B * Hkv * S * 128 / 4;
    const long long head_elems = (long long)S * 128;
    int blocks = (int)std::min<long long>(
        (n4_kv + kBlock - 1) / kBlock, kGridCap);
    dkdv_reduce_kernel<<<blocks, kBlock, 0, cur_stream()>>>(
        dk_part.data_ptr<float>(), dv_part.data_ptr<float>(), bfm(dk),
        bfm(dv), n4_kv, H / Hkv, head_elems);
    HIP_CHECK_KERNEL();
  }
  attn_bwd_dq_v2_kernel<512><<<grid, 512, DQ_DYN_LDS, cur_stream()>>>(
      bf(q), bf(k), bf(v), bf(dout), lse.data_ptr<float>(),
      delta.data_ptr<float>(), bfm(dq), B, H, Hkv, S, (float)scale,
      icausal);
  HIP_CHECK_KERNEL();
  return {dq, dk, dv};
}

// ---------------------------------------------------------- flash-decode
// The int32 [B] device vectors (lengths, pos) that the cached-attention
// kernels read and the host never does.
void check_int32_vec(const torch::Tensor& t, int B, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
              t.numel() == B && t.is_contiguous(),
              name, " must be int32 [B] on GPU");
}

// enough splits to fill 256 CUs at small B*H, chunks >= ~256 rows
int decode_splits(int B, int H, long max_len) {
  int splits = (int)std::max<long>(1, 1024 / ((long)B * H));
  splits = (int)std::min<long>(splits, (max_len + 255) / 256);
  return std::max(splits, 1);
}

// Partials, the dense (table == nullptr: kc/vc [B,Hkv,Lmax,128]) or the
// paged (kc/vc the pool) instantiation of decode.hip, and the merge.
torch::Tensor decode_launch(torch::Tensor& q, const torch::Tensor& kc,
                            const torch::Tensor& vc, const int* table,
                            const torch::Tensor& lengths, int Hkv, int Lmax,
                            int num_pages, int table_stride, int splits,
                            double scale) {
  const int B = q.size(0), H = q.size(1);
  auto f32 = q.options().dtype(torch::kFloat32);
  auto o_part = torch::empty({splits, B, H, 128}, f32);
  auto ml_part = torch::empty({splits, B, H, 2}, f32);
  auto o = torch::empty_like(q);
  dim3 grid(splits, H, B);
  if (table)
    attn_decode_paged_partial_kernel<<<grid, 256, 0, cur_stream()>>>(
        bf(q), bf(kc), bf(vc), table, lengths.data_ptr<int>(),
        o_part.data_ptr<float>(), ml_part.data_ptr<float>(), B, H, Hkv,
        num_pages, table_stride, splits, (float)scale);
  else
    attn_decode_partial_kernel<<<grid, 256, 0, cur_stream()>>>(
        bf(q), bf(kc), bf(vc), lengths.data_ptr<int>(),
        o_part.data_ptr<float>(), ml_part.data_ptr<float>(), B, H, Hkv,
        Lmax, splits, (float)scale);
  HIP_CHECK_KERNEL();
  attn_decode_merge_kernel<<<B * H, 64, 0, cur_stream()>>>(
      o_part.data_ptr<float>(), ml_part.data_ptr<float>(), bfm(o), B, H,
      splits);
  HIP_CHECK_KERNEL();
  return o;
}

torch::Tensor attn_decode_varlen(torch::Tensor q, torch::Tensor kc,
                                 torch::Tensor vc, torch::Tensor lengths,
                                 long max_len, double scale) {
  check_bf16(q, "q");
  check_bf16(kc, "kc");
  check_bf16(vc, "vc");
  const int B = q.size(0), H = q.size(1);
  const int Hkv = kc.size(1), Lmax = kc.size(2);
  TORCH_CHECK(q.size(2) == 1 && q.size(3) == 128,
              "decode expects q [B,H,1,128]");
  TORCH_CHECK(kc.size(3) == 128 && max_len >= 1 && max_len <= Lmax);
  TORCH_CHECK(H % Hkv == 0);
  check_int32_vec(lengths, B, "lengths");
  return decode_launch(q, kc, vc, nullptr, lengths, Hkv, Lmax, 0, 0,
                       decode_splits(B, H, max_len), scale);
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor kc,
                          torch::Tensor vc, long L, double scale) {
  auto lengths = torch::full({q.size(0)}, (long)L,
                             q.options().dtype(torch::kInt32));
  return attn_decode_varlen(q, kc, vc, lengths, L, scale);
}

// ------------------------------------------------------ append attention
// Sq new query rows per sequence at device-side offsets pos[b], against
// the cache rows 0 .. pos[b]+Sq-1 (append.hip). max_len bounds
// max(pos) + Sq and only sizes the split count: pos is never read here.
// The dense and the paged call share the launch plan and the launch.
struct AppendPlan {
  bool small;  // block of 1 wave, else 4
  int q_tiles;
  int splits;
};

AppendPlan append_plan(int B, int H, int Sq, long max_len) {
  // one wave (32 query rows) for the verify block, four for a chunk
  const bool small = Sq <= 32;
  const int bq = small ? 32 : 128;
  const int q_tiles = (Sq + bq - 1) / bq;
  // enough workgroups to fill 256 CUs, chunks of >= ~256 cache rows
  const long wgs = (long)B * H * q_tiles;
  int splits = (int)std::max<long>(1, (small ? 1024 : 512) / wgs);
  splits = (int)std::min<long>(splits, (max_len + 255) / 256);
  return {small, q_tiles, std::max(splits, 1)};
}

// Partials (with splits > 1), the dense (table == nullptr: kc/vc
// [B,Hkv,Lmax,128]) or the paged (kc/vc the pool) instantiation of
// append.hip at the plan's block size, and the merge.
torch::Tensor append_launch(torch::Tensor& q, const torch::Tensor& kc,
                            const torch::Tensor& vc, const int* table,
                            const torch::Tensor& pos, int Hkv, int Lmax,
                            int num_pages, int table_stride, long max_len,
                            double scale) {
  const int B = q.size(0), H = q.size(1), Sq = q.size(2);
  const AppendPlan plan = append_plan(B, H, Sq, max_len);
  const int splits = plan.splits;
  auto o = torch::empty_like(q);
  auto f32 = q.options().dtype(torch::kFloat32);
  torch::Tensor o_part, ml_part;
  float* o_part_p = nullptr;
  float* ml_part_p = nullptr;
  if (splits > 1) {
    o_part = torch::empty({splits, B, H, Sq, 128}, f32);
    ml_part = torch::empty({splits, B, H, Sq, 2}, f32);
    o_part_p = o_part.data_ptr<float>();
    ml_part_p = ml_part.data_ptr<float>();
  }
  dim3 grid(plan.q_tiles * splits, H, B);
  auto launch = [&](auto nw) {
    constexpr int NW = decltype(nw)::value;
    if (table)
      attn_append_paged_kernel<NW><<<grid, NW * WAVE, 0, cur_stream()>>>(
          bf(q), bf(kc), bf(vc), table, pos.data_ptr<int>(), bfm(o),
          o_part_p, ml_part_p, B, H, Hkv, Sq, num_pages, table_stride,
          splits, (float)scale);
    else
      attn_append_kernel<NW><<<grid, NW * WAVE, 0, cur_stream()>>>(
          bf(q), bf(kc), bf(vc), pos.data_ptr<int>(), bfm(o), o_part_p,
          ml_part_p, B, H, Hkv, Sq, Lmax, splits, (float)scale);
  };
  if (plan.small)
    launch(std::integral_constant<int, 1>{});
  else
    launch(std::integral_constant<int, 4>{});
  HIP_CHECK_KERNEL();
  if (splits > 1) {
    const long long R = (long long)B * H * Sq;
    attn_append_merge_kernel<<<(int)((R + 3) / 4), 256, 0, cur_stream()>>>(
        o_part_p, ml_part_p, bfm(o), R, splits);
    HIP_CHECK_KERNEL();
  }
  return o;
}

torch::Tensor attn_append(torch::Tensor q, torch::Tensor kc,
                          torch::Tensor vc, torch::Tensor pos,
                          long max_len, double scale) {
  check_bf16(q, "q");
  check_bf16(kc, "kc");
  check_bf16(vc, "vc");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == 128 && q.size(2) >= 1,
              "append expects q [B,H,Sq,128]");
  const int B = q.size(0), H = q.size(1);
  TORCH_CHECK(kc.dim() == 4 && kc.size(0) == B && kc.size(3) == 128,
              "append expects k_cache [B,Hkv,Lmax,128]");
  TORCH_CHECK(vc.sizes() == kc.sizes(),
              "k_cache and v_cache must have the same shape");
  const int Hkv = kc.size(1), Lmax = kc.size(2);
  TORCH_CHECK(H % Hkv == 0, "GQA requires H % Hkv == 0");
  TORCH_CHECK(max_len >= 1 && max_len <= Lmax,
              "max_len must be in [1, Lmax]");
  check_int32_vec(pos, B, "pos");
  return append_launch(q, kc, vc, nullptr, pos, Hkv, Lmax, 0, 0, max_len,
                       scale);
}

// ------------------------------------------------------- paged KV cache
// Pool [num_pages, Hkv, 64, 128] and block table int32 [B, pages_per_seq]
// (paged.hip). Neither call reads lengths / pos on the host: both are
// hipGraph-capturable.
void check_page_pool(const torch::Tensor& kp, const torch::Tensor& vp) {
  check_bf16(kp, "k_pages");
  check_bf16(vp, "v_pages");
  TORCH_CHECK(kp.dim() == 4 && kp.size(2) == PG_ROWS && kp.size(3) == PG_D,
              "page pool must be [num_pages, Hkv, 64, 128]");
  TORCH_CHECK(vp.sizes() == kp.sizes(),
              "k_pages and v_pages must have the same shape");
}

void check_block_table(const torch::Tensor& table, int B) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt32 &&
              table.dim() == 2 && table.size(0) == B &&
              table.is_contiguous(),
              "block_table must be contiguous int32 [B, pages_per_seq] "
              "on GPU");
}

torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor kp,
                                torch::Tensor vp, torch::Tensor table,
                                torch::Tensor lengths, long max_len,
                                double scale) {
  check_bf16(q, "q");
  check_page_pool(kp, vp);
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1 && q.size(3) == PG_D,
              "paged decode expects q [B,H,1,128]");
  const int B = q.size(0), H = q.size(1);
  const int num_pages = kp.size(0), Hkv = kp.size(1);
  TORCH_CHECK(H % Hkv == 0, "GQA requires H % Hkv == 0");
  check_block_table(table, B);
  const int table_stride = table.size(1);
  TORCH_CHECK(max_len >= 1 && max_len <= (long)table_stride * PG_ROWS,
              "max_len must be in [1, 64 * pages_per_seq]");
  check_int32_vec(lengths, B, "lengths");
  // the dense split count, capped by the page count: a split is whole
  // pages
  const int splits = (int)std::min<long>(
      decode_splits(B, H, max_len), (max_len + PG_ROWS - 1) / PG_ROWS);
  return decode_launch(q, kp, vp, table.data_ptr<int>(), lengths, Hkv, 0,
                       num_pages, table_stride, splits, scale);
}

// Append attention through the block table (append.hip, PAGED): Sq new
// query rows per sequence at device-side offsets pos[b] (pos[b] < 0 = the
// sequence takes no part, output 0). max_len bounds max(pos) + Sq and
// only sizes the split count: neither pos nor the table is read here.
torch::Tensor attn_append_paged(torch::Tensor q, torch::Tensor kp,
                                torch::Tensor vp, torch::Tensor table,
                                torch::Tensor pos, long max_len,
                                double scale) {
  check_bf16(q, "q");
  check_page_pool(kp, vp);
  TORCH_CHECK(q.dim() == 4 && q.size(3) == PG_D && q.size(2) >= 1,
              "paged append expects q [B,H,Sq,128]");
  const int B = q.size(0), H = q.size(1);
  const int num_pages = kp.size(0), Hkv = kp.size(1);
  TORCH_CHECK(H % Hkv == 0, "GQA requires H % Hkv == 0");
  check_block_table(table, B);
  const int table_stride = table.size(1);
  TORCH_CHECK(max_len >= 1 && max_len <= (long)table_stride * PG_ROWS,
              "max_len must be in [1, 64 * pages_per_seq]");
  check_int32_vec(pos, B, "pos");
  return append_launch(q, kp, vp, table.data_ptr<int>(), pos, Hkv, 0,
                       num_pages, table_stride, max_len, scale);
}

// k, v [B, Hkv, S, 128] may be strided views (last dim dense, 16-byte
// aligned rows): the decode step's K/V are slices of the QKV GEMM output
void check_new_rows(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16,
              name, " must be bf16 on GPU");
  TORCH_CHECK(t.dim() == 4 && t.size(3) == PG_D && t.stride(3) == 1,
              name, " must be [B,Hkv,S,128] with a dense last dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
              t.stride(2) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " rows must be 16-byte aligned");
}

void kv_page_write(torch::Tensor k, torch::Tensor v, torch::Tensor kp,
                   torch::Tensor vp, torch::Tensor table,
                   torch::Tensor pos) {
  check_new_rows(k, "k");
  check_new_rows(v, "v");
  check_page_pool(kp, vp);
  TORCH_CHECK(v.sizes() == k.sizes(), "k and v must have the same shape");
  const int B = k.size(0), Hkv = k.size(1), S = k.size(2);
  TORCH_CHECK(kp.size(1) == Hkv, "k and the pool disagree on Hkv");
  check_block_table(table, B);
  check_int32_vec(pos, B, "pos");
  const long long vecs = (long long)B * Hkv * S * (PG_D / 8);
  if (vecs == 0) return;
  kv_page_write_kernel<<<grid_for(vecs), kBlock, 0, cur_stream()>>>(
      bf(k), bf(v), bfm(kp), bfm(vp), table.data_ptr<int>(),
      pos.data_ptr<int>(), B, Hkv, S, (int)kp.size(0), (int)table.size(1),
      k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1),
      v.stride(2));
  HIP_CHECK_KERNEL();
}

// ------------------------------------------------------------ sampling
// [B, V] logits (bf16 or fp32, dense last dim, any row stride) -> int64 [B]
// token ids, every parameter per row and on the device: no host read, one
// launch (sampling.hip).
void check_row_vec(const torch::Tensor& t, int B, torch::ScalarType ty,
                   const char* name, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.dim() == 1 &&
              t.numel() == B && t.is_contiguous(),
              name, " must be ", what, " [B] on GPU");
}

torch::Tensor sample_tokens(torch::Tensor logits, torch::Tensor temperature,
                            torch::Tensor top_k, torch::Tensor top_p,
                            torch::Tensor u) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2,
              "logits must be [B, V] on GPU");
  const bool is_bf16 = logits.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(is_bf16 || logits.scalar_type() == torch::kFloat32,
              "logits must be bf16 or fp32");
  const long long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1ll << 30), "sample_tokens needs 1 <= V < 2^30");
  TORCH_CHECK(V == 1 || logits.stride(1) == 1,
              "logits must have a dense last dim");
  TORCH_CHECK(B == 1 || logits.stride(0) >= 0,
              "logits row stride must not be negative");
  check_row_vec(temperature, (int)B, torch::kFloat32, "temperature", "fp32");
  check_row_vec(top_k, (int)B, torch::kInt32, "top_k", "int32");
  check_row_vec(top_p, (int)B, torch::kFloat32, "top_p", "fp32");
  check_row_vec(u, (int)B, torch::kFloat32, "u", "fp32");
  auto out = torch::empty({B}, logits.options().dtype(torch::kInt64));
  if (B == 0) return out;
  const long long stride = B == 1 ? 0 : logits.stride(0);
  long long* outp = reinterpret_cast<long long*>(out.data_ptr<int64_t>());
  // fixed-point scale of a weight: 2^44, less where V weights of 1.0 would
  // not fit 63 bits
  int bits = 44;
  while (bits > 0 && (V >> (63 - bits)) != 0) --bits;
  const float fix = ldexpf(1.f, bits);
  if (is_bf16)
    sample_tokens_kernel<short><<<(int)B, SMP_BLOCK, 0, cur_stream()>>>(
        bf(logits), stride, (int)V, fix, temperature.data_ptr<float>(),
        top_k.data_ptr<int>(), top_p.data_ptr<float>(), u.data_ptr<float>(),
        outp);
  else
    sample_tokens_kernel<float><<<(int)B, SMP_BLOCK, 0, cur_stream()>>>(
        logits.data_ptr<float>(), stride, (int)V, fix,
        temperature.data_ptr<float>(), top_k.data_ptr<int>(),
        top_p.data_ptr<float>(), u.data_ptr<float>(), outp);
  HIP_CHECK_KERNEL();
  return out;
}

// ------------------------------------------------------- layout probes
torch::Tensor dbg_mfma32(torch::Tensor a, torch::Tensor b) {
  auto out = torch::empty({32, 32}, a.options().dtype(torch::kFloat32));
  dbg_mfma32_kernel<<<1, 64, 0, cur_stream()>>>(bf(a), bf(b),
                                                out.data_ptr<float>());
  HIP_CHECK_KERNEL();
  return out;
}

std::vector<torch::Tensor> dbg_attn_layout(torch::Tensor t,
                                           torch::Tensor x) {
  check_bf16(t, "t");
  check_bf16(x, "x");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == 64 && t.size(1) == 128,
              "t must be [64,128]");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == 32 && x.size(1) == 128,
              "x must be [32,128]");
  auto f32opts = t.options().dtype(torch::kFloat32);
  auto st = torch::empty({64, 32}, f32opts);
  auto out = torch::empty({32, 128}, f32opts);
  dbg_attn_layout_kernel<<<1, 64, 0, cur_stream()>>>(
      bf(t), bf(x), st.data_ptr<float>(), out.data_ptr<float>());
  HIP_CHECK_KERNEL();
  return {st, out};
}

std::vector<torch::Tensor> dbg_attn_image(torch::Tensor t,
                                          torch::Tensor x) {
  check_bf16(t, "t");
  check_bf16(x, "x");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == 64 && t.size(1) == 128,
              "t must be [64,128]");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == 32 && x.size(1) == 128,
              "x must be [32,128]");
  auto f32opts = t.options().dtype(torch::kFloat32);
  auto st = torch::empty({64, 32}, f32opts);
  auto out = torch::empty({32, 128}, f32opts);
  dbg_attn_image_kernel<<<1, 64, 0, cur_stream()>>>(
      bf(t), bf(x), st.data_ptr<float>(), out.data_ptr<float>());
  HIP_CHECK_KERNEL();
  return {st, out};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd, "RMSNorm forward (bf16)");
  m.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm backward");
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd, "fused residual add + RMSNorm");
  m.def("rope", &rope, "RoPE (half-rotation), fwd or bwd via sign");
  m.def("swiglu_fwd", &swiglu_fwd, "SwiGLU forward");
  m.def("swiglu_bwd", &swiglu_bwd, "SwiGLU backward");
  m.def("swiglu_gu_fwd", [](torch::Tensor gu){ return swiglu_gu_fwd(gu)[0]; }, "fused-layout SwiGLU fwd");
  m.def("swiglu_gu_bwd", &swiglu_gu_bwd, "fused-layout SwiGLU bwd");
  m.def("add_bf16", &add_bf16, "fused bf16 add");
  m.def("decode_tokens_u16", &decode_tokens_u16,
        "packed uint16 token bytes -> int64 tokens (one pass on-GPU)");
  m.def("quant_e5m2", &quant_e5m2,
        "bf16 -> OCP E5M2 bytes, one fused scale+saturate+convert pass "
        "(v_cvt_pk_bf8_f32; for delayed-scaled GRADIENT quantization)");
  m.def("quant_e4m3", &quant_e4m3,
        "one-pass bf16 -> OCP E4M3 (uint8 storage) with scale");
  m.def("adamw", &adamw, "fused AdamW (bf16 p/g, fp32 m/v[, master])");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused CE forward");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused CE backward");
  m.def("rope_qkv_fwd", &rope_qkv_fwd,
        "fused QKV split + transpose + RoPE");
  m.def("rope_qkv_bwd", &rope_qkv_bwd,
        "fused QKV rope backward -> GEMM-grad layout");
  m.def("attn_fwd", &attn_fwd, "flash attention forward (causal, GQA)");
  m.def("attn_bwd", &attn_bwd, "flash attention backward");
  m.def("attn_decode", &attn_decode,
        "split-K flash-decode over the KV cache (q [B,H,1,128])");
  m.def("attn_decode_varlen", &attn_decode_varlen,
        "flash-decode with per-sequence cache lengths (int32 [B]; "
        "length 0 = inactive slot, output 0)");
  m.def("attn_append", &attn_append,
        "append attention: Sq query rows at per-sequence offsets pos "
        "(int32 [B]) over the KV cache (q [B,H,Sq,128])");
  m.def("attn_decode_paged", &attn_decode_paged,
        "flash-decode over a paged KV cache: pool [P,Hkv,64,128], block "
        "table int32 [B,pages], lengths int32 [B] (0 = output 0)");
  m.def("attn_append_paged", &attn_append_paged,
        "append attention over a paged KV cache: q [B,H,Sq,128], pool "
        "[P,Hkv,64,128], block table int32 [B,pages], pos int32 [B] "
        "(pos < 0 = output 0)");
  m.def("kv_page_write", &kv_page_write,
        "scatter new K/V rows [B,Hkv,S,128] into the page pool at "
        "pos[b].. through the block table (pos < 0 skips the sequence)");
  m.def("sample_tokens", &sample_tokens,
        "fused sampler: logits [B,V] (bf16/fp32) + per-row temperature, "
        "top_k, top_p, u -> int64 [B] token ids (temperature <= 0 = "
        "argmax)");
  m.def("dbg_mfma32", &dbg_mfma32, "mfma 32x32x16 layout probe");
  m.def("dbg_attn_layout", &dbg_attn_layout,
        "attention panel / transposed-read / col_to_afrags layout probe");
  m.def("dbg_attn_image", &dbg_attn_image,
        "train kernels' dual-use LDS image: staging / row-read / "
        "transposed-read probe");
}
