"""Shared by the loaders' slot-reuse tests: a way to keep the consumer stream behind the host."""
import torch


def busy(dev, state={}):
    """Queue some tens of milliseconds of work on the current stream, so that what is launched next is still waiting while the host
    goes on (a chain of 4096 x 4096 fp32 products, 137 GFLOP each)."""
    if "a" not in state:
        state["a"] = torch.randn((4096, 4096), device=dev) / 64
    x = state["a"]
    for _ in range(12):
        x = x @ state["a"]
    return x
