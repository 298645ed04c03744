"""Drop-in for the reference's `emd_cuda` extension (models/EMD/cuda/emd.cpp:24-26) on the HIP kernels.

`mocopci_amd.compat.install()` registers it as `sys.modules["emd_cuda"]`, so the reference's models/EMD/emd.py imports and
differentiates unchanged.  Same names, argument orders and result shapes as the pybind module:
    approxmatch_forward(xyz1 (B,N,3), xyz2 (B,M,3)) -> match (B,M,N)
    matchcost_forward(xyz1, xyz2, match) -> cost (B)
    matchcost_backward(grad_cost (B), xyz1, xyz2, match) -> [grad1 (B,N,3), grad2 (B,M,3)]
float32 CUDA tensors only."""
from .emd import approxmatch_forward, matchcost_backward, matchcost_forward

__all__ = ["approxmatch_forward", "matchcost_forward", "matchcost_backward"]
