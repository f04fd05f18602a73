"""What every call into libvsscore.so does to its arguments, once: plain functions and one context manager.
The C call itself stays at its call site and reads as the prototype does."""
from __future__ import annotations

import ctypes as C

import torch


def ptr(t):
    """device address of a tensor, None (a NULL argument) for None"""
    return None if t is None else t.data_ptr()


def mask_u8(mask):
    """None, or the mask as contiguous uint8: a view of a bool mask, a copy of any other dtype"""
    if mask is None:
        return None
    m = mask.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


def host_lengths(lengths):
    """(list of int, the same values as the host int32 array the packed entry points take)"""
    lengths = [int(t) for t in lengths]
    return lengths, (C.c_int32 * len(lengths))(*lengths)


def scratch(nbytes: int, device, floor: int = 0):
    """uninitialised device bytes for a workspace / record of ``nbytes`` (a size query's answer), at least ``floor``"""
    return torch.empty((max(int(nbytes), floor),), dtype=torch.uint8, device=device)


def stream_of(device) -> int:
    """raw handle of ``device``'s current stream - for a call that already runs with ``device`` current"""
    return torch.cuda.current_stream(device).cuda_stream


class on_stream(torch.cuda.device):
    """``with on_stream(dev) as stream:`` - ``torch.cuda.device(dev)`` that also hands out the raw handle of ``dev``'s current
    stream (no generator behind it: the small calls enter it several times per step)"""

    def __enter__(self) -> int:
        self.prev_idx = torch.cuda._exchange_device(self.idx)       # torch.cuda.device.__enter__, without a second frame
        return torch.cuda.current_stream(self.idx).cuda_stream
