"""Numerics tests for the gfx950 HIP kernels vs plain PyTorch fp32
references. All @pytest.mark.gpu — run on the MI355X box."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def setup_module():
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built+loadable on GPU"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-8)).item()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def test_rmsnorm_fwd_bwd(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    x = torch.randn(512, 4096, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    w = torch.randn(4096, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    y = K.rmsnorm(x, w)
    xr = x.detach().clone().float().requires_grad_(True)
    wr = w.detach().clone().float().requires_grad_(True)
    yr = K.rmsnorm_ref(xr, wr)
    assert rel_err(y, yr) < 2e-2

    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    assert rel_err(x.grad, xr.grad) < 2e-2
    assert rel_err(w.grad, wr.grad) < 2e-2


def test_rope_fwd_bwd(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    B, S, H, D = 2, 256, 4, 128
    cos_t, sin_t = K.rope_tables(S, D, device=dev)
    x = torch.randn(B, S, H, D, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    y = K.rope(x, cos_t, sin_t)
    xr = x.detach().clone().requires_grad_(True)
    yr = K.rope_ref(xr, cos_t, sin_t)
    assert rel_err(y, yr) < 2e-2
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy)
    assert rel_err(x.grad, xr.grad) < 2e-2


def test_swiglu_fwd_bwd(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    g = torch.randn(1024, 1024, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    u = torch.randn_like(g, requires_grad=True)
    y = K.swiglu(g, u)
    gr = g.detach().clone().float().requires_grad_(True)
    ur = u.detach().clone().float().requires_grad_(True)
    yr = torch.nn.functional.silu(gr) * ur
    assert rel_err(y, yr) < 2e-2
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    assert rel_err(g.grad, gr.grad) < 2e-2
    assert rel_err(u.grad, ur.grad) < 2e-2


def test_cross_entropy(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    N, V = 512, 32000
    logits = torch.randn(N, V, dtype=torch.bfloat16, device=dev,
                         requires_grad=True)
    tgt = torch.randint(0, V, (N,), device=dev)
    loss = K.cross_entropy(logits, tgt)
    lr_ = logits.detach().clone().float().requires_grad_(True)
    loss_ref = torch.nn.functional.cross_entropy(lr_, tgt, reduction="none")
    assert rel_err(loss, loss_ref) < 1e-2

    loss.mean().backward()
    loss_ref.mean().backward()
    assert rel_err(logits.grad, lr_.grad) < 2e-2


def test_adamw(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    n = 8192
    p = torch.randn(n, dtype=torch.bfloat16, device=dev)
    g = torch.randn(n, dtype=torch.bfloat16, device=dev)
    m = torch.zeros(n, dtype=torch.float32, device=dev)
    v = torch.zeros(n, dtype=torch.float32, device=dev)
    p_ref = p.clone().float().cpu()
    g_ref = g.clone().float().cpu()
    m_ref = torch.zeros(n)
    v_ref = torch.zeros(n)

    for step in (1, 2, 3):
        K.adamw_step(p, g, m, v, step, lr=1e-3)
        gf = g_ref
        m_ref.mul_(0.9).add_(gf, alpha=0.1)
        v_ref.mul_(0.95).addcmul_(gf, gf, value=0.05)
        c1 = 1 / (1 - 0.9 ** step)
        c2 = 1 / (1 - 0.95 ** step)
        p_ref -= 1e-3 * ((m_ref * c1) / ((v_ref * c2).sqrt() + 1e-8)
                         + 0.1 * p_ref)
        # bf16 roundtrip to mirror kernel state
        p_ref = p_ref.to(torch.bfloat16).float()
    assert rel_err(p.float().cpu(), p_ref) < 2e-2
    assert rel_err(m.cpu(), m_ref) < 1e-2
    assert rel_err(v.cpu(), v_ref) < 1e-2


@pytest.mark.parametrize("B,H,Hkv,S", [
    (1, 2, 2, 256),     # MHA
    (2, 4, 1, 256),     # GQA 4:1
    (1, 8, 2, 512),     # GQA 4:2
    (1, 4, 2, 257),     # unaligned: padded to 512 internally
    (2, 4, 1, 100),     # unaligned, S < one tile
    (1, 4, 4, 320),     # 64-aligned but not 256-aligned
])
def test_attention_fwd(dev, B, H, Hkv, S):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    q = torch.randn(B, H, S, 128, dtype=torch.bfloat16, device=dev)
    k = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev)
    v = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev)
    o = K.attention(q, k, v)
    o_ref = K.attention_ref(q, k, v)
    assert rel_err(o, o_ref) < 2e-2, "fwd mismatch"


@pytest.mark.parametrize("B,H,Hkv,S", [
    pytest.param(1, 4, 2, 256, id="256"),
    pytest.param(1, 4, 2, 257, id="257"),
    pytest.param(1, 4, 2, 100, id="100"),
    # B>1 and G=4 partial-slot indexing, two kv blocks x several q tiles
    pytest.param(2, 8, 2, 512, id="b2-g4-512"),
])
def test_attention_bwd(dev, B, H, Hkv, S):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    q = torch.randn(B, H, S, 128, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    k = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    v = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    o = K.attention(q, k, v)
    dout = torch.randn_like(o)
    o.backward(dout)

    qr = q.detach().clone().float().requires_grad_(True)
    kr = k.detach().clone().float().requires_grad_(True)
    vr = v.detach().clone().float().requires_grad_(True)
    o_ref = K.attention_ref(qr, kr, vr)
    o_ref.backward(dout.float())
    assert rel_err(q.grad, qr.grad) < 3e-2, "dq"
    assert rel_err(k.grad, kr.grad) < 3e-2, "dk"
    assert rel_err(v.grad, vr.grad) < 3e-2, "dv"


def test_rope_qkv_fused(dev):
    """Fused QKV split+transpose+RoPE vs the torch composition (which the
    CPU fallback implements), forward and backward."""
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(5)
    B, S, nq, nkv = 2, 256, 4, 2
    qkv = torch.randn(B, S, (nq + 2 * nkv) * 128, dtype=torch.bfloat16,
                      device=dev, requires_grad=True)
    cos_t, sin_t = K.rope_tables(S, 128, 500000.0, device=dev)
    q, k, v = K.rope_qkv(qkv, cos_t, sin_t, nq, nkv)
    dq, dk, dv = (torch.randn_like(q), torch.randn_like(k),
                  torch.randn_like(v))
    torch.autograd.backward([q, k, v], [dq, dk, dv])
    g_fused = qkv.grad.clone()

    qkv2 = qkv.detach().cpu().requires_grad_(True)
    q2, k2, v2 = K.rope_qkv(qkv2, cos_t.cpu(), sin_t.cpu(), nq, nkv)
    torch.autograd.backward([q2, k2, v2],
                            [dq.cpu(), dk.cpu(), dv.cpu()])
    for name, got, want in (("q", q, q2), ("k", k, k2), ("v", v, v2),
                            ("dqkv", g_fused, qkv2.grad)):
        assert rel_err(got, want.to(dev)) < 2e-2, name


def test_attention_noncausal(dev):
    """Non-causal kernel path (causal=0 in attention.hip) — the
    off-diagonal chunk op of ring attention (parallel/ring_attention.py):
    fwd o + lse and all three grads vs the fp32 reference."""
    import math

    from metaflow_amd.ops import kernels as K

    torch.manual_seed(3)
    B, H, Hkv, S = 1, 4, 2, 512
    scale = 1.0 / math.sqrt(128)
    q = torch.randn(B, H, S, 128, dtype=torch.bfloat16, device=dev)
    k = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev)
    v = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16, device=dev)
    o, lse = K.attn_fwd_raw(q, k, v, scale, causal=False)
    oc, lsec = K.attn_fwd_raw(q.cpu(), k.cpu(), v.cpu(), scale,
                              causal=False)
    assert rel_err(o, oc.to(dev)) < 2e-2, "fwd o"
    assert (lse - lsec.to(dev)).abs().max().item() < 1e-2, "fwd lse"

    dout = torch.randn_like(o)
    dq, dk, dv = K.attn_bwd_raw(q, k, v, o, dout, lse, scale, causal=False)
    dqc, dkc, dvc = K.attn_bwd_raw(q.cpu(), k.cpu(), v.cpu(), oc,
                                   dout.cpu(), lsec, scale, causal=False)
    assert rel_err(dq, dqc.to(dev)) < 3e-2, "dq"
    assert rel_err(dk, dkc.to(dev)) < 3e-2, "dk"
    assert rel_err(dv, dvc.to(dev)) < 3e-2, "dv"


def test_tiny_model_step(dev):
    """One full train step of the tiny model: loss finite, grads flow,
    fused adam updates params."""
    import torch

    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from metaflow_amd.parallel.ddp import FlatParamModel, FusedAdamW

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=2048, seq=256)
    model = LlamaForCausalLM(cfg).to(dev)
    flat = FlatParamModel(model)
    opt = FusedAdamW(flat, lr=1e-3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 257), device=dev)
    losses = []
    for _ in range(8):
        flat.zero_grad()
        loss = model(tokens[:, :-1], tokens[:, 1:].contiguous())
        loss.backward()
        flat.finish_grad_sync()
        opt.step()
        losses.append(float(loss.item()))
    assert all(l == l for l in losses), "NaN loss"
    assert losses[-1] < losses[0], "loss did not decrease: %s" % losses


def test_mixtral_tiny_step(dev):
    """One train step of the tiny Mixtral (dense single-rank MoE path on
    the HIP kernels): finite decreasing loss, router + experts get grads."""
    import torch

    from metaflow_amd.models.mixtral import MixtralConfig, MixtralForCausalLM
    from metaflow_amd.parallel.ddp import FlatParamModel, FusedAdamW

    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=2048, seq=256)
    model = MixtralForCausalLM(cfg).to(dev)
    flat = FlatParamModel(model)
    opt = FusedAdamW(flat, lr=1e-3)
    tokens = torch.randint(0, cfg.vocab_size, (2, 257), device=dev)
    losses = []
    for _ in range(8):
        flat.zero_grad()
        loss = model(tokens[:, :-1], tokens[:, 1:].contiguous())
        loss.backward()
        flat.finish_grad_sync()
        opt.step()
        losses.append(float(loss.item()))
    assert all(l == l for l in losses), "NaN loss"
    assert losses[-1] < losses[0], "loss did not decrease: %s" % losses


@pytest.mark.parametrize("prompt_len", [256, 200])
def test_generate_gpu(dev, prompt_len):
    """KV-cache decode on hardware: flash-kernel prefill (any prompt
    length — unaligned seqlens are padded to the 256-tile internally) +
    cached decode; greedy tokens must match the uncached full forward
    (which itself exercises the padded attention path at every t)."""
    import torch

    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=256, seq=512)
    m = LlamaForCausalLM(cfg).to(dev).eval()
    torch.manual_seed(1)
    prompt = torch.randint(0, 256, (1, prompt_len), device=dev)
    out = m.generate(prompt, 4)
    assert out.shape == (1, prompt_len + 4)
    with torch.no_grad():
        for t in range(prompt_len, prompt_len + 4):
            full = m(out[:, :t])
            nxt = full[:, -1].float().argmax(-1)
            assert torch.equal(nxt, out[:, t]), t


def test_swiglu_fused(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    gu = torch.randn(512, 2048, dtype=torch.bfloat16, device=dev,
                     requires_grad=True)
    y = K.swiglu_fused(gu)
    gr = gu.detach().clone().float().requires_grad_(True)
    I = 1024
    yr = torch.nn.functional.silu(gr[..., :I]) * gr[..., I:]
    assert rel_err(y, yr) < 2e-2
    dy = torch.randn_like(y)
    y.backward(dy)
    yr.backward(dy.float())
    assert rel_err(gu.grad, gr.grad) < 2e-2


def test_mfma32_layout_probe(dev):
    """Regression guard for the 32x32x16 fragment layout every v2 kernel
    assumes (asymmetric inputs per guide G9: transpose-detecting)."""
    from metaflow_amd.ops import kernels as K

    ext = K.hip_ext()
    torch.manual_seed(3)
    a = torch.randn(32, 16, dtype=torch.bfloat16, device=dev)
    b = torch.randn(16, 32, dtype=torch.bfloat16, device=dev)
    c = ext.dbg_mfma32(a, b)
    ref = a.float() @ b.float()
    assert rel_err(c, ref) < 1e-3


def test_attn_layout_probe(dev):
    """Isolation guard for the attention kernels' layout chain, run through
    the production helpers: panel staging, panel A-fragments, the
    C-column -> A-fragment repack and the hardware-transposed B-fragment
    reads. Inputs from {-1, 0, 1}: x·t^T holds integers of magnitude
    <= 128 (exact in bf16) and the second product integers <= 8192 (exact
    in fp32), so both outputs must EQUAL the fp32 matmul; x and t are
    independent, so a transposed or permuted layout cannot pass."""
    from metaflow_amd.ops import kernels as K

    ext = K.hip_ext()
    g = torch.Generator().manual_seed(7)
    tf = torch.randint(-1, 2, (64, 128), generator=g).float()
    xf = torch.randint(-1, 2, (32, 128), generator=g).float()
    st, out = ext.dbg_attn_layout(tf.to(dev, torch.bfloat16),
                                  xf.to(dev, torch.bfloat16))
    assert torch.equal(st.cpu(), tf @ xf.T)
    assert torch.equal(out.cpu(), (xf @ tf.T) @ tf)


def test_add_rmsnorm_fused(dev):
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    x = torch.randn(256, 4096, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    r = torch.randn_like(x, requires_grad=True)
    w = torch.randn(4096, dtype=torch.bfloat16, device=dev,
                    requires_grad=True)
    s, y = K.add_rmsnorm(x, r, w)
    xr = x.detach().clone().float().requires_grad_(True)
    rr = r.detach().clone().float().requires_grad_(True)
    wr = w.detach().clone().float().requires_grad_(True)
    sr = xr + rr
    yr = K.rmsnorm_ref(sr, wr)
    assert rel_err(s, sr) < 2e-2
    assert rel_err(y, yr) < 2e-2
    # both outputs used downstream (like the model: s -> residual, y -> op)
    ds = torch.randn_like(s)
    dy = torch.randn_like(y)
    (s * ds + y * dy).sum().backward()
    (sr * ds.float() + yr * dy.float()).sum().backward()
    assert rel_err(x.grad, xr.grad) < 2e-2
    assert rel_err(r.grad, rr.grad) < 2e-2
    assert rel_err(w.grad, wr.grad) < 2e-2


def test_tuned_linear_gpu(dev, tmp_path, monkeypatch):
    """End-to-end tuned GEMM path: search winners for a small shape in
    all three modes (fwd/dx/dw), pin them via a table file, and check
    TunedLinear's forward AND gradients against torch."""
    import json

    from metaflow_amd.ops import _mfx_gemm as G
    from metaflow_amd.ops import gemm

    torch.manual_seed(0)
    M, K, N = 512, 256, 384
    x0 = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.1
    w0 = torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.1
    dy = torch.randn(M, N, dtype=torch.bfloat16, device=dev) * 0.1
    table = {}
    for mode, mid, a, b in (("fwd", 0, w0, x0), ("dx", 1, w0, dy),
                            ("dw", 2, x0, dy)):
        idxs, ms = G.search(mid, a, b, 2, 16)
        assert idxs.numel() > 0
        table["%s|%d,%d,%d" % (mode, M, K, N)] = int(idxs[0])
    f = tmp_path / "table.json"
    f.write_text(json.dumps(table))
    monkeypatch.setenv("MFX_GEMM_TUNE_FILE", str(f))
    gemm.reset_tune_table()
    try:
        x = x0.clone().requires_grad_(True)
        w = w0.clone().requires_grad_(True)
        out = gemm.tuned_linear(x, w)
        out.backward(dy)

        xr = x0.clone().requires_grad_(True)
        wr = w0.clone().requires_grad_(True)
        ref = torch.nn.functional.linear(xr, wr)
        ref.backward(dy)
        assert rel_err(out, ref) < 2e-2, "fwd"
        assert rel_err(x.grad, xr.grad) < 2e-2, "dx"
        assert rel_err(w.grad, wr.grad) < 2e-2, "dw"
    finally:
        gemm.reset_tune_table()


@pytest.mark.parametrize("B,H,Hkv,L", [
    (1, 4, 2, 257),     # unaligned cache length, GQA
    (2, 8, 8, 1000),    # MHA, bigger cache
    (1, 4, 1, 64),      # small L (single split)
])
def test_attn_decode(dev, B, H, Hkv, L):
    """Split-K flash-decode vs the fp32 reference: one query per head
    against the first L cache positions (full cache stride, GQA)."""
    import math

    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    Lmax = L + 37  # cache longer than the valid prefix
    q = torch.randn(B, H, 1, 128, dtype=torch.bfloat16, device=dev)
    kc = torch.randn(B, Hkv, Lmax, 128, dtype=torch.bfloat16,
                     device=dev)
    vc = torch.randn(B, Hkv, Lmax, 128, dtype=torch.bfloat16,
                     device=dev)
    scale = 1.0 / math.sqrt(128)
    o = K.attn_decode(q, kc, vc, L, scale)
    ref = K.attention_ref(q, kc[:, :, :L], vc[:, :, :L], scale,
                          causal=False)
    assert o.shape == (B, H, 1, 128)
    assert rel_err(o, ref) < 2e-2


def test_fp8_linear_gpu(dev):
    """E4M3 GEMM numerics (fp8 tolerance vs the bf16 product) and the
    delayed-scaling Fp8Linear module's fwd/bwd."""
    from metaflow_amd.ops.fp8 import E4M3_MAX, Fp8Linear, quantize_e4m3
    from metaflow_amd.ops import _mfx_gemm as G

    torch.manual_seed(0)
    M, K, N = 512, 256, 384
    x = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.1
    w = torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.1
    sx = E4M3_MAX / x.abs().max().float().item()
    sw = E4M3_MAX / w.abs().max().float().item()
    got = G.fp8(quantize_e4m3(x, sx), quantize_e4m3(w, sw),
                1.0 / (sx * sw))
    ref = torch.nn.functional.linear(x, w)
    assert rel_err(got, ref) < 6e-2

    lin = Fp8Linear(K, N).to(dev)
    with torch.no_grad():
        lin.weight.copy_(w)
    xg = x.clone().requires_grad_(True)
    out0 = lin(xg)          # step 1: bf16 warmup, fills history
    out1 = lin(xg)          # step 2: fp8 path
    assert rel_err(out1, ref) < 6e-2
    out1.sum().backward()
    assert xg.grad is not None and lin.weight.grad is not None


def test_fp8_bwd_linear_gpu(dev):
    """fp8_bwd=True: dgrad AND wgrad through the E4M3 GEMM (delayed-
    scaled dy, byte-transposed operands) match the bf16 autograd
    gradients to fp8 tolerance."""
    from metaflow_amd.ops.fp8 import Fp8Linear

    torch.manual_seed(1)
    M, K, N = 512, 256, 384
    x = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.1
    w = torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.1
    dy = torch.randn(M, N, dtype=torch.bfloat16, device=dev) * 1e-3

    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    torch.nn.functional.linear(xr, wr).backward(dy)

    lin = Fp8Linear(K, N, fp8_bwd=True).to(dev)
    with torch.no_grad():
        lin.weight.copy_(w)
    xg = x.clone().requires_grad_(True)
    lin(xg)                         # bf16 warmup step
    out = lin(xg)                   # fp8 fwd + fp8 bwd
    out.backward(dy)
    assert rel_err(xg.grad, xr.grad) < 8e-2
    assert rel_err(lin.weight.grad, wr.grad) < 8e-2
    # second backward uses the RECORDED dy amax (delayed scaling)
    assert float(lin.amax_dy.max()) > 0
    xg2 = x.clone().requires_grad_(True)
    lin(xg2).backward(dy)
    assert rel_err(xg2.grad, xr.grad) < 8e-2


def test_attn_decode_varlen_gpu(dev):
    """Varlen flash-decode: per-slot lengths (incl. an inactive slot)
    vs the per-slot fp32 reference."""
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    B, H, Hkv, Lmax = 4, 8, 2, 700
    q = torch.randn(B, H, 1, 128, dtype=torch.bfloat16, device=dev)
    kc = torch.randn(B, Hkv, Lmax, 128, dtype=torch.bfloat16,
                     device=dev)
    vc = torch.randn_like(kc)
    lengths = [513, 0, 699, 64]
    o = K.attn_decode_varlen(q, kc, vc, lengths, 0.0883)
    assert torch.all(o[1] == 0)
    for b in (0, 2, 3):
        ref = K.attention_ref(q[b:b + 1], kc[b:b + 1, :, :lengths[b]],
                              vc[b:b + 1, :, :lengths[b]], 0.0883,
                              causal=False)
        assert rel_err(o[b:b + 1], ref) < 2e-2, b


def test_continuous_batching_gpu(dev):
    """Serving engine on hardware: greedy tokens from the batcher
    (varlen decode kernel, slots at different positions) match
    per-request generate()."""
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from metaflow_amd.serving import ContinuousBatcher

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=256, seq=512)
    m = LlamaForCausalLM(cfg).to(dev).eval()
    prompts = [([5, 9, 17, 4], 6), (list(range(2, 40)), 5),
               ([100, 101], 8), ([7] * 21, 4)]
    batcher = ContinuousBatcher(m, max_batch=2, max_len=128)
    reqs = [batcher.submit(p, n) for p, n in prompts]
    out = batcher.run()
    for req, (prompt, n) in zip(reqs, prompts):
        ref = m.generate(torch.tensor([prompt], device=dev),
                         n)[0, len(prompt):].tolist()
        assert out[req.id] == ref, (req.id, out[req.id], ref)


def test_checkpoint_stream_roundtrip_gpu(dev, tmp_path):
    """GPU checkpoint through the pipelined save_stream path (D2H
    double-buffered halves -> Merkle leaves -> CAS) restores exact
    bytes, and the key dedups against the non-streamed path."""
    from metaflow_amd.datastore import FlowDataStore
    from metaflow_amd.datastore.storage import LocalStorage
    from metaflow_amd.parallel.checkpoint import (
        load_state_dict,
        save_state_dict,
    )

    fds = FlowDataStore("CkptFlow", LocalStorage(str(tmp_path)))
    ds = fds.get_task_datastore("1", "train", "t", attempt=0, mode="w")
    ds.init_task()
    torch.manual_seed(0)
    state = {
        "big": torch.randn(96 << 20, dtype=torch.bfloat16,
                           device=dev),  # 192 MiB: Merkle regime
        "small": torch.randn(1000, dtype=torch.float32, device=dev),
        "step": 3,
    }
    index = save_state_dict(ds, state, name="s")
    ds.done()
    rd = fds.get_task_datastore("1", "train", "t")
    out = load_state_dict(rd, name="s", map_location=dev)
    assert out["step"] == 3
    for k in ("big", "small"):
        assert torch.equal(out[k], state[k]), k
    # cross-path dedup: saving the same content CPU-side hits the key
    from metaflow_amd.datastore.cas import parallel_key

    cpu_bytes = state["big"].cpu().reshape(-1).view(
        torch.uint8).numpy().tobytes()
    assert parallel_key(cpu_bytes) == index["big"]["sha"]


def test_quant_e4m3_kernel(dev):
    """One-pass quantize kernel vs the torch composition (bitwise —
    both saturate to +-448 and round-to-nearest-even)."""
    from metaflow_amd.ops.fp8 import E4M3_MAX
    from metaflow_amd.ops.kernels import hip_ext

    torch.manual_seed(0)
    x = torch.randn(4096, 512, dtype=torch.bfloat16, device=dev) * 3
    x[0, 0] = 10000.0   # saturation
    x[0, 1] = -10000.0
    scale = 7.5
    got = hip_ext().quant_e4m3(x, scale)
    ref = ((x.float() * scale).clamp(-E4M3_MAX, E4M3_MAX)
           .to(torch.float8_e4m3fn).view(torch.uint8))
    mismatch = (got != ref).float().mean().item()
    assert mismatch < 1e-3, mismatch  # allow boundary rounding ties


def test_decode_tokens_u16(dev):
    """On-GPU uint16 token decode matches the numpy view (2 B/token over
    the bus instead of 8)."""
    from metaflow_amd.ops import kernels as K

    torch.manual_seed(0)
    toks = torch.randint(0, 65536, (1 << 16,), dtype=torch.int32)
    raw = toks.to(torch.int16).view(torch.uint8)
    got = K.decode_tokens_u16(raw.to(dev))
    want = K.decode_tokens_u16(raw)
    assert got.dtype == torch.int64
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want, toks.to(torch.int64))


def test_continuous_batching_mixtral_gpu(dev):
    """MoE serving on hardware: batcher tokens match per-request
    Mixtral generate() (eager decode; graph capture correctly skipped
    for the shape-dynamic router)."""
    from metaflow_amd.models.mixtral import (
        MixtralConfig,
        MixtralForCausalLM,
    )
    from metaflow_amd.serving import ContinuousBatcher

    torch.manual_seed(0)
    m = MixtralForCausalLM(
        MixtralConfig.tiny(vocab=256, seq=256)).to(dev).eval()
    batcher = ContinuousBatcher(m, max_batch=2, max_len=64)
    assert batcher._graph is None  # MoE: no capture
    prompts = [([5, 9, 17, 4], 5), (list(range(2, 20)), 4)]
    reqs = [batcher.submit(p, n) for p, n in prompts]
    out = batcher.run()
    for req, (prompt, n) in zip(reqs, prompts):
        ref = m.generate(torch.tensor([prompt], device=dev),
                         n)[0, len(prompt):].tolist()
        assert out[req.id] == ref, (req.id, out[req.id], ref)


def test_fp8_with_recompute_gpu(dev):
    """Fp8Linear under activation checkpointing: the recompute must
    reuse the original forward's scales and touch no amax state
    (otherwise the recomputed activations diverge from what autograd
    saved — this crashed bench --fp8 --recompute)."""
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=128, seq=128)
    cfg.fp8 = True
    cfg.recompute = True
    m = LlamaForCausalLM(cfg).to(dev)
    toks = torch.randint(0, 128, (2, 65), device=dev)
    for _ in range(3):  # past the bf16 warmup step into the fp8 path
        loss = m(toks[:, :-1], toks[:, 1:].contiguous())
        m.zero_grad(set_to_none=True)
        loss.backward()
    assert torch.isfinite(loss).item()
    # amax history advanced once per forward, not per recompute
    probe = m.layers[0].qkv_proj
    assert probe._step == 3
