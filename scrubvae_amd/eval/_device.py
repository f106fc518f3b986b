"""What the eval modules share about the device: which one a call runs on, how an array gets there, and the host clock their
timings read."""
import time

import torch


def _device_of(*arrays, who):
    """the device of the first of `arrays` that is a device tensor, else the current one; `who` is the RuntimeError's sentence
    when there is none"""
    for x in arrays:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise RuntimeError(who)
    return torch.device("cuda", torch.cuda.current_device())


def _on_device(a, dev):
    """a (numpy or torch) as a contiguous tensor on dev"""
    if not torch.is_tensor(a):
        a = torch.from_numpy(a if a.flags.writeable else a.copy())  # torch refuses to share a read-only array
    return a.to(dev).contiguous()


def _clock(device, sync=True):
    """the host clock once everything queued on `device` is done; sync=False: the clock alone (nobody asked for the timing)"""
    if sync:
        torch.cuda.synchronize(device)
    return time.perf_counter()
