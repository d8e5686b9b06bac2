"""Weight-only FP8 expert weights on the CPU: the row quantiser, the
quantised expert module and the E4M3 MoeTable. The kernels are tested in
test_moe_fp8_gpu.py."""

import pytest
import torch

from metaflow_amd.models.mixtral import MixtralConfig, MoELayer
from metaflow_amd.ops import kernels as K


def _weights(E, hidden, inter, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [[(0.05 * torch.randn(shape, generator=g)).to(torch.bfloat16)
             for _ in range(E)]
            for shape in ((inter, hidden), (inter, hidden), (hidden, inter))]


def test_quantiser_rounds_within_half_a_step():
    g = torch.Generator().manual_seed(1)
    # rows of very different size, one all zero, one with a lone element
    w = torch.randn(40, 256, generator=g) * \
        (2.0 ** torch.arange(-20, 20).float())[:, None]
    w[7] = 0
    w[9, 1:] = 0
    w8, scale = K.moe_quant_weight(w)
    assert w8.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert scale[7] == 1.0 and (w8[7].float() == 0).all()
    torch.testing.assert_close(scale[9], w[9, 0].abs() / 448, rtol=1e-6,
                               atol=0)
    v = (w / scale[:, None]).abs().double()
    assert v.max() <= 448 * (1 + 1e-6)
    # E4M3 spacing at |v|: 2^(e - 3) in the binade 2^e, 2^-9 below 2^-6;
    # RNE errs by at most half of it (2^-20: the fp32 division before it)
    step = 2.0 ** (torch.floor(torch.log2(v.clamp_min(2.0 ** -6))) - 3)
    err = (K.moe_dequant_ref(w8, scale, torch.float64) - w.double()).abs()
    assert (err <= 0.5 * step * scale[:, None].double() * (1 + 2.0 ** -20)
            ).all()


def test_state_dict_round_trips_a_quantised_layer():
    cfg = MixtralConfig.tiny()
    torch.manual_seed(0)
    layer = MoELayer(cfg)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=0.05)
    x = torch.randn(1, 6, cfg.hidden_size).to(torch.bfloat16)
    layer.quantize_experts_()
    assert layer.quantized
    assert [n for n, _ in layer.named_parameters()] == ["router.weight"]
    other = MoELayer(cfg).quantize_experts_()
    other.load_state_dict(layer.state_dict())
    for (n, a), (_, b) in zip(layer.named_buffers(), other.named_buffers()):
        assert a.dtype == b.dtype, n
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), n
    with torch.no_grad():
        assert torch.equal(layer(x), other(x))


def test_table_refuses_mixed_dtypes_and_missing_scales():
    ws = _weights(2, 128, 128)
    q = [[K.moe_quant_weight(w) for w in m] for m in ws]
    w8 = [[p[0] for p in m] for m in q]
    scales = [[p[1] for p in m] for m in q]
    assert K.MoeTable(*w8, scales=scales).fp8 and not K.MoeTable(*ws).fp8
    with pytest.raises(ValueError, match="mix"):
        K.MoeTable(w8[0], ws[1], w8[2], scales=scales)
    with pytest.raises(ValueError, match="need scales"):
        K.MoeTable(*w8)
    with pytest.raises(ValueError, match="scales go with"):
        K.MoeTable(*ws, scales=scales)
    with pytest.raises(ValueError, match="out rows"):
        K.MoeTable(*w8, scales=[scales[0], scales[1],
                                [s[:-1] for s in scales[2]]])


def test_cpu_ffn_is_the_reference_on_dequantised_weights():
    E, k, hidden, inter, T = 4, 2, 128, 256, 9
    q = [[K.moe_quant_weight(w) for w in m] for m in _weights(E, hidden,
                                                              inter)]
    table = K.MoeTable(*[[p[0] for p in m] for m in q],
                       scales=[[p[1] for p in m] for m in q])
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, hidden, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, generator=g)
    deq = [[K.moe_dequant_ref(*p) for p in m] for m in q]
    want = K.moe_ffn_ref(x, logits, *deq, k).to(torch.bfloat16)
    assert torch.equal(K.moe_ffn(x, logits, table, top_k=k), want)
