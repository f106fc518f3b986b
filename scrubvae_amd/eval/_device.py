"""What the eval modules share about the device: which one a call runs on, and the host clock their timings read."""
import time

import torch


def _device_of(x, who):
    """the device of x if it is a device tensor, else the current one; `who` is the RuntimeError's sentence when there is none"""
    if torch.is_tensor(x) and x.is_cuda:
        return x.device
    if not torch.cuda.is_available():
        raise RuntimeError(who)
    return torch.device("cuda", torch.cuda.current_device())


def _clock(device, sync=True):
    """the host clock once everything queued on `device` is done; sync=False: the clock alone (nobody asked for the timing)"""
    if sync:
        torch.cuda.synchronize(device)
    return time.perf_counter()
