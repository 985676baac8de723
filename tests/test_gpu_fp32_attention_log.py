"""GPU suite of hriemo_attn_probs_varlen_log_fp32 beside the other fp32-mode kernel suites: the fp32 export into an attention log is the kernel of hriemo_attn_probs_f32_varlen with another store address, so its
limit is bit equality with that entry -- which test_gpu_fp32_attention_kernels.py holds to the float64 limits.  The operands, the
guarded log and the windows are those of tests/test_gpu_attention_log_kernels.py, here at the head widths 32, 64 and 128 that file
leaves out."""
import pytest
import torch

import test_gpu_attention_log_kernels as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_f32_export_into_the_log_equals_the_plain_export(hd):
    ref = K.operands(True, hd)[5]
    for what, (slot0, n_take) in K.WINDOWS.items():
        buf, log = K.guarded(K.OUT[0] * K.OUT[1])
        window = torch.tensor([slot0, n_take, 0, 0], dtype=torch.int32, device="cuda")
        assert K.export_log(True, hd, log, window) == 0, what
        torch.cuda.synchronize()
        K.check(buf, ref, slot0, n_take, (what, hd))
