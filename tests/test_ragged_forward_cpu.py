"""-m "not gpu": the ragged forward on the CPU reference backend (tests/ragged_backend.py: every length-taking operator runs the
oracle on each element's live prefix alone and pads with zeros), and the argument validation of the lengths.

A padded batch of two samples with l1[b] = l2[b] (N = 1400, lengths 1400 and 1150, NaN padding) against the dense forward of each
cropped pair on the plain oracle backend: harness_checks.frame_deviation inside the budgets test_config4_model_runs_at_full_batch...
uses for batch-8 against batch-1 (elem <= 0.02, POINT_BUDGET, MAX_DISP_BUDGET, MSE_BUDGET), padded rows exact zeros, the sampled
pyramid exact.  The same seeds and lengths serve the comparison of the HIP forward with this reference in test_ragged_forward_gpu.py.
Validation: a wrong count, a negative length, a length above N, a wrong number of gt_lengths, and a prefetch handle's record of its
lengths (lengths_key: what _consume_prefetched compares)."""
import pytest
import torch

from mocopci_amd import model as M, ops, synth
from tests import harness_checks as hc
from tests.ragged_backend import RaggedBackend
from oracle.backend import OracleBackend

N, LENS = 1400, (1400, 1150)


def ragged_case(device="cpu"):
    x1, x2, _ = synth.make_batch(6, 2, N, device=device)   # the seeds of forward_b2_n2048, where the suite holds the HIP forward to the CPU side
    for b, l in enumerate(LENS):
        x1[b, :, l:], x2[b, :, l:] = float("nan"), float("nan")
    return x1, x2


def test_ragged_forward_is_each_cloud_alone_on_the_reference_backend():
    net = hc.build_model("cpu")
    x1, x2 = ragged_case()
    prev = ops.set_backend(RaggedBackend())
    try:
        got = net(x1, x2, lengths1=LENS, lengths2=LENS)
        pcs_g, _ = net.run_encoder(torch.nan_to_num(torch.cat([x1, x2]).transpose(1, 2).contiguous()), lengths=LENS + LENS)
        ops.set_backend(OracleBackend())
        for b, l in enumerate(LENS):
            c1, c2 = x1[b:b + 1, :, :l].contiguous(), x2[b:b + 1, :, :l].contiguous()
            want = net(c1, c2)
            for j, (o, w) in enumerate(zip(got, want)):
                elem, pts, worst, mse = hc.frame_deviation(o[b:b + 1, :l].numpy(), w.numpy())
                line = f"sample {b} (length {l}), frame {j}: coords off {elem:.4%}, points moved {pts:.4%}, worst {worst:.3g} x spread, mse {mse:.3g} x spread^2"
                print(line)
                assert elem <= 0.02 and pts <= hc.POINT_BUDGET and worst <= hc.MAX_DISP_BUDGET and mse <= hc.MSE_BUDGET, line
                assert (o[b, l:] == 0).all()
            pcs_w, _ = net.run_encoder(torch.cat([c1, c2]).transpose(1, 2).contiguous())
            for lvl in range(1, 5):
                assert torch.equal(pcs_g[lvl][b], pcs_w[lvl][0]) and torch.equal(pcs_g[lvl][2 + b], pcs_w[lvl][1]), (b, lvl)
    finally:
        ops.set_backend(prev)


def test_lengths_are_validated():
    net = hc.build_model("cpu")
    x1, x2, gt = synth.make_batch(2, 2, 256)
    prev = ops.set_backend(RaggedBackend())
    try:
        for bad in ([256], [256, 256, 256], [-1, 256], [256, 257], [1.5, 2.0]):
            with pytest.raises(RuntimeError, match="lengths"):
                net(x1, x2, lengths1=bad)
            with pytest.raises(RuntimeError, match="lengths"):
                net(x1, x2, lengths2=bad)
        with pytest.raises(RuntimeError, match="gt_lengths"):
            net(x1, x2, [g.transpose(1, 2).contiguous() for g in gt], None, True, lengths1=[256, 200], gt_lengths=[[256, 256]])
    finally:
        ops.set_backend(prev)


def test_a_prefetch_handle_remembers_its_lengths():
    key = M.MoCoPCI.lengths_key
    assert key(None, None) == (None, None) and key([5, 7], None) == ((5, 7), None)
    assert key(torch.tensor([5, 7]), (1, 2)) == ((5, 7), (1, 2)) and key([5, 7], None) != key([5, 6], None) != key(None, [5, 6])
    net = hc.build_model("cpu")
    x1, x2, _ = synth.make_batch(2, 1, 64)
    handle = {"lengths": key([64], None), "lens": None, "inputs": (x1.data_ptr(), x2.data_ptr(), tuple(x1.shape)), "versions": (0, 0), "stream": 0,
              "sched": None, "scope": {}}
    with pytest.raises(RuntimeError, match="other lengths"):
        net._consume_prefetched(handle, x1, x2, [63], None)
    with pytest.raises(RuntimeError, match="other lengths"):
        net._consume_prefetched(handle, x1, x2, None, None)
