"""One-wave GPU probe of the train kernels' dual-use LDS image, run through
the production helpers (stage_image, img_row_frag, acc_to_bfrags,
img_tr_load): dbg_attn_image_kernel stages a [64][128] tile t, forms
S^T = t·x^T from row reads, then O^T = t^T·bf16(S^T) from hardware-
transposed reads of the same copy.

Inputs from {-1, 0, 1}: t·x^T holds integers of magnitude <= 128 (exact in
bf16) and the second product integers <= 8192 (exact in fp32), so both
outputs must EQUAL the fp32 matmul. t and x are independent, so a
transposed, permuted or chunk-swapped layout cannot pass.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [7, 8])
def test_attn_image_probe(seed):
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built+loadable on GPU"
    ext = K.hip_ext()
    g = torch.Generator().manual_seed(seed)
    tf = torch.randint(-1, 2, (64, 128), generator=g).float()
    xf = torch.randint(-1, 2, (32, 128), generator=g).float()
    st, out = ext.dbg_attn_image(tf.cuda().to(torch.bfloat16),
                                 xf.cuda().to(torch.bfloat16))
    assert torch.equal(st.cpu(), tf @ xf.T)
    assert torch.equal(out.cpu(), (xf @ tf.T) @ tf)
