"""-m gpu: the software-pipelined fusion_split_kernel (csrc/fusion.hip: the ReLU + operand split of one 32-neighbour chain runs in the
MFMA gaps of the other) computes the bits the kernel computed before the pipeline.

(a) Stored bits.  The sha256 of be.fusion_mlp's output bytes on the seeded inputs of tests/fused_reference.fusion_inputs is compared with
tests/golden/fusion_forward_sha256.json, which was recorded ONCE with the library of the commit before the pipeline:

    MCP_HIP_LIB=<libmocopci_hip.so of the parent commit> python -m tests.test_fusion_pipeline_gpu --record

Totals of 1, 3, 5 and 2 x 1500 points and 4 * 4096 + 5 points (the capped grid of 4096 workgroups, whose second round is ragged: one
workgroup of each of the first seven XCD eighths comes back for four more points), each with the neighbour list as two (B,N,32) halves and
as one (B,N,64) list, and each once more with the second half a repeat of the first (duplicate indices).  The kernel takes one point per
wave per round, so there is no total at which a wave pipelines across points.

(b) Float64.  The large total once more against fused_reference.fusion_reference at test_fused_variants_gpu.C_FUSION, on the first and
last 64 points of every round of every eighth and 512 seeded points."""
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from mocopci_amd import ops  # noqa: E402
from tests import fused_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(HERE, "golden", "fusion_forward_sha256.json")
WAVES, GRID_CAP = 4, 4096          # fusion.hip: WAVES, grid_cap of mcp_fusion
BIG = 4 * GRID_CAP + 5
TOTALS = [(1, 1), (1, 3), (1, 5), (2, 1500), (1, BIG)]
CASES = [dict(b=b, n=n, dup=dup) for b, n in TOTALS for dup in (False, True)]


def case_id(c):
    return f"{c['b']}x{c['n']}" + ("-dup" if c["dup"] else "")


_inputs = {}


def inputs(case):
    key = case_id(case)
    if key not in _inputs:
        p1, p2, idx, ws = fr.fusion_inputs(case)
        _inputs[key] = (p1, p2, idx, ws)
    return _inputs[key]


def run(case, form):
    p1, p2, (ia, ib), ws = inputs(case)
    d = [t.to(DEV) for t in (p1, p2, ia, ib, *ws)]
    idx = (d[2], d[3]) if form == "two" else torch.cat([d[2], d[3]], -1)
    return ops.backend().fusion_mlp(d[0], d[1], idx, *d[4:])


def digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("form", ["two", "one"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fusion_bits_are_the_stored_bits(case, form):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = run(case, form)
    assert torch.isfinite(got).all()
    assert digest(got) == golden[f"{case_id(case)}/{form}"], "the output bits differ from the ones recorded before the pipeline"


def round_edges(total):
    """Flat indices of the first and last 64 points of every round of every XCD eighth (mcp_units_by_xcd, common.h) at the capped grid."""
    grid = min((total + WAVES - 1) // WAVES, GRID_CAP)
    assert grid % 8 == 0
    steps = (total + WAVES - 1) // WAVES
    chunk, stride = (steps + 7) // 8 * WAVES, grid // 8 * WAVES
    sel = []
    for x in range(8):
        lim = min((x + 1) * chunk, total)
        lo = x * chunk
        while lo < lim:
            hi = min(lo + stride, lim)
            sel += list(range(lo, min(lo + 64, hi))) + list(range(max(hi - 64, lo), hi))
            lo = hi
    return sel


@pytest.mark.parametrize("dup", [False, True], ids=["", "dup"])
def test_fusion_big_total_matches_float64(dup):
    from tests.test_fused_variants_gpu import C_FUSION
    case = dict(b=1, n=BIG, dup=dup)
    p1, p2, idx, ws = inputs(case)
    got = run(case, "two").reshape(-1, 3).double().cpu()
    g = torch.Generator().manual_seed(7)
    sel = torch.tensor(sorted(set(round_edges(BIG)) | set(torch.randint(0, BIG, (512,), generator=g).tolist())))
    exact, bound = fr.fusion_reference(p1, p2, idx, *ws, sel=sel)
    ratio = ((got[sel] - exact).abs() / (C_FUSION * fr.U * bound).clamp_min(1e-300)).max().item()
    print(f"RATIO fusion-pipeline[{case_id(case)}] kernel={ratio:.3f} over {sel.numel()} points")
    assert ratio <= 1.0, f"fusion_split_kernel: error {ratio:.2f} x the bound"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    out = {f"{case_id(c)}/{form}": digest(run(c, form)) for c in CASES for form in ("two", "one")}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} digests with {os.environ.get('MCP_HIP_LIB', 'the built library')}")
