"""-m gpu: the MoCoPCI forward on padded batches with per-cloud lengths (MoCoPCI.forward / prefetch / begin / finish / run_encoder
with lengths1 / lengths2, training.multiscale_loss with lengths).  Stress weights (harness_checks.build_model).

  (a) full lengths give the bits of the forward without lengths, through forward() and through begin() / finish() with a prefetched
      handle, at B = 2, N = 2048 and at B = 1, N = 8192 (the pruned length searches and the one-launch PointConv);
  (b) padding independence: l1 = (2048, 1500), l2 = (1301, 2048), the padding filled with NaN, with 7.5 and with a copy of live points:
      equal bits on live rows, exact zeros on padded rows;
  (c) other samples: another content and length of sample 1, length 0 included, leaves every bit of sample 0;
  (d) the cloud alone: a sample with l1 = l2 = L, L = 1500 and 5000 padded to 8192, against the dense forward on the cropped pair,
      harness_checks.frame_deviation inside the budgets test_config4_model_runs_at_full_batch... uses for batch-8 against batch-1
      (elem <= 0.02, POINT_BUDGET, MAX_DISP_BUDGET, MSE_BUDGET); the sampled pyramids of run_encoder(lengths=) are exact;
  (f) the budgets bite: the same padded batch WITHOUT lengths misses at least one of them;
  (g) the training forward after net.train() with the dropout rates at 0, B = 2, N = 1024, lengths (1024, 700) / (900, 1024): the loss
      and every gradient are finite, the gradients of the inputs are exact zeros on padded columns, and every parameter gradient and
      the fusion BatchNorm's running estimates are equal bits under finite and under NaN padding;
  and a prefetch handle made under other lengths is refused.
  (e) different lengths of the two frames, l1 = (2048, 1500), l2 = (1301, 2048) with NaN padding, against the CPU reference of the
      ragged forward (tests/ragged_backend.py), same budgets.  The input is the one batch at which the suite already holds the DENSE
      HIP forward to the CPU side (forward_b2_n2048: synth.make_batch(6, 2, 2048)), the seeds of test_ragged_forward_cpu.py: a
      HIP-against-CPU comparison says something about the lengths only where the dense one is inside its budgets, and at an
      arbitrary seed it is not (make_batch(2, 1, 1400), no lengths anywhere: frame 0 has 20 % of its coordinates off, mse 3.0e-5)."""
import pytest
import torch

from mocopci_amd import synth, training
from tests import harness_checks as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net():
    return hc.build_model(DEV)


def padded(x, lens, fill):
    """x (B,3,N) with the columns at or beyond lens[b] replaced: a number, or "copy" = live points again."""
    x = x.clone()
    for b, l in enumerate(lens):
        n = x.shape[2] - l
        if n == 0:
            continue
        if fill == "copy":
            x[b, :, l:] = x[b, :, torch.arange(n, device=x.device) % max(l, 1)] if l else 1.25
        else:
            x[b, :, l:] = fill
    return x


def check_frames(out, want, l1, l2, what):
    for j, (o, w) in enumerate(zip(out, want)):
        for b, l in enumerate(l1 if j < 2 else l2):
            assert torch.equal(o[b, :l], w[b, :l]), f"{what}: frame {j}, sample {b}: live rows differ"
            assert (o[b, l:] == 0).all(), f"{what}: frame {j}, sample {b}: padded rows are not exact zeros"


@pytest.mark.parametrize("b,n", [(2, 2048), (1, 8192)])
def test_full_lengths_are_the_forward_without_lengths(net, b, n):
    x1, x2, _ = synth.make_batch(2, b, n, device=DEV)
    want = net(x1, x2)
    full = [n] * b
    for name, got in (("forward", net(x1, x2, lengths1=full, lengths2=full)), ("one length given", net(x1, x2, lengths2=full)),
                      ("device lengths", net(x1, x2, lengths1=torch.tensor(full, device=DEV, dtype=torch.int32)))):
        for u, v in zip(got, want):
            assert torch.equal(u, v), f"{name}: full lengths differ from the forward without lengths"
    h = net.prefetch(x1, x2, lengths1=full, lengths2=full)
    got = net.finish(net.begin(x1, x2, prefetched=h, lengths1=full, lengths2=full))
    for u, v in zip(got, want):
        assert torch.equal(u, v), "begin / finish with a prefetched handle: full lengths differ from the forward without lengths"
    h = net.prefetch(x1, x2, lengths1=full, lengths2=full)
    with pytest.raises(RuntimeError, match="other lengths"):
        net(x1, x2, prefetched=h, lengths1=[n - 1] * b, lengths2=full)
    torch.cuda.synchronize()


L1, L2 = (2048, 1500), (1301, 2048)


@pytest.fixture(scope="module")
def ragged_pair():
    x1, x2, _ = synth.make_batch(2, 2, 2048, device=DEV)
    return x1, x2


def test_padding_reaches_nothing(net, ragged_pair):
    x1, x2 = ragged_pair
    runs = [net(padded(x1, L1, f), padded(x2, L2, f), lengths1=L1, lengths2=L2) for f in (float("nan"), 7.5, "copy")]
    for out in runs:
        assert all(torch.isfinite(o).all() for o in out)
        check_frames(out, runs[0], L1, L2, "padding")
    via = net.finish(net.begin(padded(x1, L1, 7.5), padded(x2, L2, 7.5), lengths1=L1, lengths2=L2))
    check_frames(via, runs[0], L1, L2, "begin / finish")


def test_other_samples_change_no_bit(net, ragged_pair):
    x1, x2 = ragged_pair
    base = net(padded(x1, L1, 0.5), padded(x2, L2, 0.5), lengths1=L1, lengths2=L2)
    y1, y2, _ = synth.make_batch(3, 2, 2048, device=DEV)
    for l1b, l2b in ((900, 333), (0, 0), (0, 2048)):
        z1, z2 = x1.clone(), x2.clone()
        z1[1], z2[1] = y1[1], y2[1]
        l1, l2 = (L1[0], l1b), (L2[0], l2b)
        out = net(padded(z1, l1, float("nan")), padded(z2, l2, float("nan")), lengths1=l1, lengths2=l2)
        for j, (o, w) in enumerate(zip(out, base)):
            assert torch.isfinite(o).all()
            assert torch.equal(o[0], w[0]), f"sample 1 with lengths ({l1b}, {l2b}) changed frame {j} of sample 0"
            assert (o[1, (l1b if j < 2 else l2b):] == 0).all()


@pytest.mark.parametrize("L", [1500, 5000])
def test_a_padded_sample_is_the_cloud_alone(net, L):
    N = 8192
    x1, x2, _ = synth.make_batch(2, 1, N, device=DEV)
    c1, c2 = x1[:, :, :L].contiguous(), x2[:, :, :L].contiguous()
    want = net(c1, c2)
    p1, p2 = padded(x1, (L,), float("nan")), padded(x2, (L,), float("nan"))
    got = net(p1, p2, lengths1=[L], lengths2=[L])
    blind = net(padded(x1, (L,), 7.5), padded(x2, (L,), 7.5))          # the same padded batch without lengths
    inside = lambda e, p, w, m: e <= 0.02 and p <= hc.POINT_BUDGET and w <= hc.MAX_DISP_BUDGET and m <= hc.MSE_BUDGET
    missed = False
    for j, (o, w, bl) in enumerate(zip(got, want, blind)):
        dev = hc.frame_deviation(o[:, :L].cpu().numpy(), w.cpu().numpy())
        print(f"L = {L}, frame {j}, padded with lengths vs the cloud alone: coords off {dev[0]:.4%}, points moved {dev[1]:.4%}, "
              f"worst {dev[2]:.3g} x spread, mse {dev[3]:.3g} x spread^2")
        assert inside(*dev), (L, j, dev)
        assert (o[:, L:] == 0).all()
        devb = hc.frame_deviation(bl[:, :L].cpu().numpy(), w.cpu().numpy())
        print(f"L = {L}, frame {j}, padded WITHOUT lengths: coords off {devb[0]:.4%}, points moved {devb[1]:.4%}, worst {devb[2]:.3g}, mse {devb[3]:.3g}")
        missed = missed or not inside(*devb)
    assert missed, "the budgets do not bite: padding that enters the searches, the sampling and the statistics stays inside them"
    # the sampled pyramids are exactly the cloud's own
    lay = lambda a, b: torch.cat([a, b], dim=0).transpose(1, 2).contiguous()
    pcs_w, _ = net.run_encoder(lay(c1, c2))
    pcs_g, _ = net.run_encoder(torch.nan_to_num(lay(p1, p2), nan=0.0), lengths=[L, L])
    for lvl in range(1, 5):
        assert torch.equal(pcs_g[lvl], pcs_w[lvl]), f"level {lvl} of the sampled pyramid differs from the cloud's own"


def test_training_forward_on_a_padded_batch():
    net = hc.build_model(DEV)
    net.train()
    net.drop_rate = net.attn_drop_rate = net.drop_path_rate = 0.0
    B, N, l1, l2 = 2, 1024, (1024, 700), (900, 1024)
    x1, x2, gt = synth.make_batch(2, B, N, device=DEV)
    gt = [g.transpose(1, 2).contiguous() for g in gt]
    state = {k: v.clone() for k, v in net.state_dict().items()}
    results = []
    for fill in (0.5, float("nan")):
        net.load_state_dict(state)
        a, b = padded(x1, l1, fill).requires_grad_(True), padded(x2, l2, fill).requires_grad_(True)
        ff, fb, gtf, out = net(a, b, gt, None, True, lengths1=l1, lengths2=l2)
        loss, _ = training.multiscale_loss(ff, fb, gtf, out, gt, lengths1=l1, lengths2=l2)
        params = [p for p in net.parameters() if p.requires_grad]
        grads = torch.autograd.grad(loss, [a, b] + params, allow_unused=True)
        assert torch.isfinite(loss)
        for g in grads:
            assert g is None or torch.isfinite(g).all()
        for g, l in ((grads[0], l1), (grads[1], l2)):
            for s, n in enumerate(l):
                assert (g[s, :, n:] == 0).all(), "the gradient of an input is not zero on padded columns"
        check_frames(out, out, l1, l2, "training forward")
        results.append((loss.detach(), grads[2:], {k: v.clone() for k, v in net.state_dict().items() if "running" in k}))
    (la, ga, ra), (lb, gb, rb) = results
    assert torch.equal(la, lb)
    for u, v in zip(ga, gb):
        assert (u is None and v is None) or torch.equal(u, v), "a parameter gradient depends on the padding"
    for k in ra:
        assert torch.equal(ra[k], rb[k]), f"{k} depends on the padding"


def test_different_lengths_match_the_reference_backend(net):
    from mocopci_amd import ops
    from tests.ragged_backend import RaggedBackend
    l1, l2 = L1, L2
    x1, x2, _ = synth.make_batch(6, 2, 2048, device=DEV)
    x1, x2 = padded(x1, l1, float("nan")), padded(x2, l2, float("nan"))
    got = net(x1, x2, lengths1=l1, lengths2=l2)
    cpu_net = hc.build_model("cpu")
    prev = ops.set_backend(RaggedBackend())
    try:
        want = cpu_net(x1.cpu(), x2.cpu(), lengths1=l1, lengths2=l2)
    finally:
        ops.set_backend(prev)
    for j, (o, w) in enumerate(zip(got, want)):
        for b, l in enumerate(l1 if j < 2 else l2):
            elem, pts, worst, mse = hc.frame_deviation(o[b:b + 1, :l].cpu().numpy(), w[b:b + 1, :l].numpy())
            line = f"frame {j}, sample {b} (length {l}) vs the CPU reference: coords off {elem:.4%}, points moved {pts:.4%}, worst {worst:.3g} x spread, mse {mse:.3g} x spread^2"
            print(line)
            assert elem <= 0.02 and pts <= hc.POINT_BUDGET and worst <= hc.MAX_DISP_BUDGET and mse <= hc.MSE_BUDGET, line
            assert (o[b, l:] == 0).all()
