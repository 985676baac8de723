"""CPU suite of hri_emo_amd.optim.DeviceAdamW: what can be said without a GPU -- it is a torch Optimizer, and gradient buckets that
live in host memory are refused loudly instead of being handed to torch.optim.AdamW behind the caller's back."""
import pytest
import torch


def test_device_adamw_refuses_cpu_buckets_loudly():
    import hri_emo_amd as H
    from hri_emo_amd.dp import GradBuckets
    from hri_emo_amd.optim import DeviceAdamW
    assert issubclass(DeviceAdamW, torch.optim.Optimizer) and DeviceAdamW._step_supports_amp_scaling
    m = H.FusionWithEmotionDecoder(d_model=128, num_emotions=4)
    buckets = GradBuckets(m.parameters(), overlap=False)
    homes = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceAdamW(buckets)
    assert homes == [p.data_ptr() for p in m.parameters()], "a refused construction must not have moved the parameters"
