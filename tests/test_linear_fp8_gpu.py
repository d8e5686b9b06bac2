"""The stream kernels of linear_fp8.hip on the GPU: K.linear_w8 against the
fp64 reference on the exactly dequantised weights (K.linear_w8_ref), at the
smallest shapes that reach each branch (a single chunk, odd chunk counts, one
chunk per split, a full token block, a second block and a second group with
a few rows, SwiGLU finished in the kernel and after the split sum, both weight
types), and the captured serving step of a quantised Llama.

The bound: the worst per-row relative L2 error must come within 2x of what
the dequantising fallback (bf16 weights, a bf16 GEMM, K.swiglu_fused) makes
of the same inputs. Row r of the weight is multiplied by 2 ** ((5 r) % 7 - 3)
before quantising, so a wrong row-to-scale pairing through the C layout, or a
wrong gate/up pairing at r and inter + r, is a gross error. Measured (kernel
/ fallback) are printed and recorded in docs/KERNELS.md."""

import pytest
import torch

from metaflow_amd.models import llama
from metaflow_amd.ops import kernels as K

from .test_moe_prefill_gpu import _worst_row_err

pytestmark = pytest.mark.gpu

F8, BF = torch.float8_e4m3fn, torch.bfloat16


def setup_module():
    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


# (M, K, N or inter, swiglu, splits, weight dtype)
CASES = [
    (1, 128, 128, False, 1, F8),      # one chunk: the self-prefetch edge
    (5, 384, 256, False, 1, F8),      # an odd chunk count
    (5, 384, 256, False, 3, F8),      # one chunk per split
    (32, 256, 128, False, 1, F8),     # a full block
    (33, 256, 128, False, 1, F8),     # a second block with one row
    (64, 256, 256, False, None, F8),  # a full group, the split rule
    (70, 384, 128, False, 1, F8),     # a second group with 6 rows
    (5, 256, 256, True, 1, F8),       # SwiGLU finished in the kernel
    (5, 256, 256, True, 2, F8),       # SwiGLU after the split sum
    (40, 384, 256, True, 1, F8),
    (5, 384, 256, False, 3, BF),
    (40, 384, 256, True, 1, BF),
]


@pytest.mark.parametrize(
    "M,kdim,n,swiglu,splits,wdtype", CASES,
    ids=["M%d-K%d-N%d-%s-s%s-%s" % (c[0], c[1], c[2],
                                    "swiglu" if c[3] else "plain", c[4],
                                    "fp8" if c[5] == F8 else "bf16")
         for c in CASES])
def test_linear_w8(dev, M, kdim, n, swiglu, splits, wdtype):
    g = torch.Generator().manual_seed(M + kdim)
    rows = 2 * n if swiglu else n
    w = 0.05 * torch.randn(rows, kdim, generator=g) * \
        (2.0 ** ((5 * torch.arange(rows)) % 7 - 3))[:, None]
    if wdtype == F8:
        w, scale = K.moe_quant_weight(w)
        w, scale = w.to(dev), scale.to(dev)
        wb = K.linear_dequant(w, scale)
        assert torch.equal(wb.cpu(), K.moe_dequant_ref(w.cpu(), scale.cpu(),
                                                       BF))
    else:
        w, scale = w.to(BF).to(dev), None
        wb = w
    big = torch.full((M + 2, kdim), float("nan"), dtype=BF)
    big[1:M + 1] = torch.randn(M, kdim, generator=g).to(BF)
    x = big.to(dev)[1:M + 1]   # inside a NaN-filled allocation
    ref = K.linear_w8_ref(x.cpu(), w.cpu(),
                          None if scale is None else scale.cpu(), swiglu)

    def run(x):
        return K.linear_w8(x, w, scale, swiglu=swiglu, splits=splits)

    out, again = run(x), run(x)
    fallback = torch.nn.functional.linear(x, wb)
    if swiglu:
        fallback = K.swiglu_fused(fallback)
    assert out.shape == (M, n) and out.dtype == BF
    assert torch.equal(out, again)
    err, fb_err = _worst_row_err(out, ref), _worst_row_err(fallback, ref)
    print("M=%d K=%d N=%d swiglu=%d splits=%s %s worst per-row rel L2: "
          "kernel %.3e, fallback %.3e"
          % (M, kdim, n, swiglu, splits, wdtype, err, fb_err))
    assert err <= 2 * fb_err

    # the same rows in another order (13 is coprime to every M here): a
    # row's result does not depend on its place in a group
    perm = ((13 * torch.arange(M) + 3) % M).to(dev)
    assert torch.equal(run(x[perm].contiguous()), out[perm])


def test_serving_captures_fp8_llama(dev):
    torch.manual_seed(0)
    # inter 640: 5 chunks, the odd tail of the unrolled loop in down_proj
    cfg = llama.LlamaConfig(vocab_size=512, hidden_size=256,
                            intermediate_size=640, num_layers=2, num_heads=2,
                            num_kv_heads=1, head_dim=128, max_seq_len=256)
    m = llama.LlamaForCausalLM(cfg).to(dev).eval().quantize_weights_()
    assert m.graph_safe_decode and isinstance(m.lm_head,
                                              llama.Fp8WeightLinear)
    from metaflow_amd.serving import ContinuousBatcher

    # the long prompt prefills through the dequantising fallback
    long = [(7 * i + 3) % 512 for i in range(llama.STREAM_MAX_ROWS + 6)]
    prompts = [([5, 9, 17, 4], 5), (long, 4)]
    outs = []
    for graph in (True, False):
        b = ContinuousBatcher(m, max_batch=2, max_len=192, graph=graph)
        assert (b._graph is not None) == graph
        reqs = [b.submit(p, n) for p, n in prompts]
        res = b.run()
        outs.append([res[r.id] for r in reqs])
    assert outs[0] == outs[1]
    assert [len(o) for o in outs[0]] == [n for _, n in prompts]
