"""-m "not gpu": the fusion layer's length forms (csrc/fusion_lengths.hip, the kept-score pair of csrc/fusion_bn_lengths.hip), what
can be held without a device.

  * The four entry points are declared in the header with `const int *len` behind idx2 and the dense parameters around it, carry
    the dense signature plus the added pointers in _lib.SIGNATURES, and are exported.
  * Argument validation returns before anything is launched, with the dense entries' codes: a NULL pointer or a non-positive
    dimension is MCP_ERR_BAD_ARG, nb != 64 MCP_ERR_UNSUPPORTED, a workspace that is too small MCP_ERR_BAD_ARG -- with lengths and
    with len = NULL (the dense entry itself)."""
import os
import re

import pytest

from mocopci_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED = 10001, 10002
# new entry -> (the dense entry it follows, the parameters it adds, in order)
NEW = {
    "mcp_fusion_lengths": ("mcp_fusion", ["const int *len"]),
    "mcp_fusion_grad_lengths": ("mcp_fusion_grad", ["const int *len"]),
    "mcp_fusion_bn_forward_save_lengths": ("mcp_fusion_bn_forward_save", ["const int *len", "int *count"]),
    "mcp_fusion_bn_backward_saved_lengths": ("mcp_fusion_bn_backward_saved", ["const int *len"]),
}


def declared_parameters(name):
    text = open(os.path.join(ROOT, "include", "mocopci_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % name, text, re.S | re.M)
    assert m, f"{name} is not declared in include/mocopci_hip.h"
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_entry_point_is_declared_bound_and_exported(name):
    dense, added = NEW[name]
    params = declared_parameters(name)
    assert params[7] == "const int *len" and params[6] == "const int *idx2", params[:8]
    assert [p for p in params if p not in added] == declared_parameters(dense), "the dense parameters, in the dense order"
    assert len(params) == len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[dense]) + len(added)
    assert _lib.SIGNATURES[name][:7] == _lib.SIGNATURES[dense][:7]
    assert hasattr(_lib.load(), name), f"{name} is not exported"


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    p = 16   # any non-null, 16-byte aligned address: nothing is launched
    for ln in (p, None):   # with lengths, and len = NULL: the dense entry and so its errors
        fwd = lambda b=1, nb=64, p1=p, out=p: lib.mcp_fusion_lengths(b, 1, nb, p1, p, p, p, ln, p, p, p, p, p, p, out, None)
        assert fwd(p1=None) == BAD and fwd(out=None) == BAD and fwd(b=0) == BAD
        assert fwd(nb=32) == UNSUPPORTED and fwd(nb=65) == UNSUPPORTED
        bwd = lambda b=1, nb=64, g=p, w3=p, ws=p, size=1 << 30: lib.mcp_fusion_grad_lengths(b, 1, nb, p, p, p, p, ln, p, p, p, p, w3, p, g, p, p, p, ws, size, None)
        assert bwd(g=None) == BAD and bwd(ws=None) == BAD and bwd(b=0) == BAD
        assert bwd(w3=p + 4) == BAD             # W3 rows are read as float4
        assert bwd(nb=32) == UNSUPPORTED
        assert bwd(size=0) == BAD               # workspace too small
        assert bwd(size=lib.mcp_fusion_grad_workspace_bytes(1, 1) - 1) == BAD
        save = lambda nb=64, sc=p, size=1 << 30: lib.mcp_fusion_bn_forward_save_lengths(1, 1, nb, p, p, p, p, ln, p, p, p, p, p, p, 1e-3, p, p, p, p, sc, p, p, p,
                                                                                        size, None)
        assert save(sc=None) == BAD and save(nb=32) == UNSUPPORTED and save(size=0) == BAD
        saved = lambda nb=64, sz=p, size=1 << 30: lib.mcp_fusion_bn_backward_saved_lengths(1, 1, nb, p, p, p, p, ln, p, p, p, p, p, p, p, p, p, sz, p, p, p, p, p,
                                                                                           p, p, p, p, p, p, size, None)
        assert saved(sz=None) == BAD and saved(nb=32) == UNSUPPORTED and saved(size=0) == BAD
