"""Which GPU kernels a call launched (torch.profiler), for tests that must tell a fast path from its fallback."""
import torch


def launched(fn):
    """-> (fn(), set of the names of the GPU kernels it launched)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA}


def ran(names, kernel):
    return any(kernel in n for n in names)
