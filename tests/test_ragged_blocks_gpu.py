"""-m gpu: the two train-mode attention blocks on a padded batch.  MoCoPCI.cross_frame_att(lengths=) on x (2,2,40,256) and
MoCoPCI.multi_frame_att_full(lengths=) on x (2,5,40,64), lens (40, 23), in a net.train() forward without dropout (net._mode =
(0, 0, 0), net._live as forward sets it): the BatchNorms run on the live rows' statistics (csrc/bn_batch.hip), the attention gets the
lengths for queries and keys.  Padding is finite garbage (7.5); the upstream gradient is zero on padded rows.

Live rows of both outputs, the gradient of x on live rows, every parameter gradient of the block and the norm layers' running
estimates are compared against the same block run per sample on the cropped cloud, on a second copy of the model (parameter
gradients summed over the samples, running estimates after the samples in sequence); num_batches_tracked must be equal.
ratio = max|ragged - per sample| / (BOUND * max|per sample|) <= 1 for every tensor.  Two gradients of multi_frame_att_full are zero
in exact arithmetic and have no max-abs of their own to be measured by: attn_feats.proj.bias and the value half of attn_feats.kv.bias
shift a channel of norm2's input by a constant, which its batch statistics remove, and the key half shifts every score of a softmax
row alike.  What both runs return there is rounding residue of sums over the rows whose weighted forms are the same layer's weight
gradient, so these two are measured by that weight gradient's max-abs (ZERO_EXACT).  BOUND: the smallest power of two at least twice
the worst ratio measured on the MI355X (in brackets; every RATIO line: profiles/bn_batch_accuracy.txt).  The bound must bite: the
same call on the padded batch with the lengths omitted misses it by more than 10x."""
import pytest
import torch

from tests import harness_checks as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2.0 ** -14      # [2.05e-5: multi_frame_att_full, d norm1.bias]
LENS = (40, 23)
N = 40
ZERO_EXACT = {"multi_frame_att_full": {"attn_feats.proj.bias": "attn_feats.proj.weight", "attn_feats.kv.bias": "attn_feats.kv.weight"}}
BLOCKS = {
    "cross_frame_att": ("multi_frame_inference.cross_block3", (2, 2, N, 256)),
    "multi_frame_att_full": ("multi_frame_inference.multi_frame_up_1.cross_block", (2, 5, N, 64)),
}


class train_forward:
    """What MoCoPCI.forward sets around a net.train() forward without dropout."""

    def __init__(self, net, mode=(0.0, 0.0, 0.0)):
        self.net, self.mode = net, mode

    def __enter__(self):
        self.net._live = {**dict(self.net.named_parameters()), **dict(self.net.named_buffers())}
        self.net._mode = self.mode
        return self.net

    def __exit__(self, *exc):
        self.net._live = None
        self.net._mode = None


def run(net, which, prefix, x, ups, **kw):
    """-> (outputs, gradient of x, {name: parameter gradient})"""
    params = {k: p for k, p in net.named_parameters() if k.startswith(prefix + ".")}
    x = x.clone().requires_grad_(True)
    with train_forward(net):
        outs = getattr(net, which)(prefix, x, **kw)
        grads = torch.autograd.grad(outs, [x, *params.values()], ups, allow_unused=True)
    return [o.detach() for o in outs], grads[0], {k: g for k, g in zip(params, grads[1:]) if g is not None}


def estimates(net, prefix):
    return {k: b.clone() for k, b in net.named_buffers() if k.startswith(prefix + ".norm")}


@pytest.mark.parametrize("which", list(BLOCKS))
def test_a_block_on_a_padded_batch_gives_what_it_gives_for_each_cloud_alone(which):
    prefix, shape = BLOCKS[which]
    net, alone = hc.build_model(DEV), hc.build_model(DEV)
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(*shape, generator=gen).to(DEV)
    live = (torch.arange(N).view(1, N) < torch.tensor(LENS).view(2, 1)).to(DEV)            # (2, N)
    x[~live.view(2, 1, N, 1).expand_as(x)] = 7.5
    before = estimates(net, prefix)
    with torch.no_grad(), train_forward(net):
        shapes = [tuple(o.shape) for o in getattr(net, which)(prefix, x)]
        for k, b in net.named_buffers():    # the probe moved the running estimates
            if k in before:
                b.copy_(before[k])
    ups = [torch.randn(*s, generator=gen).to(DEV) * live.view(2, 1, N, 1) for s in shapes]

    outs, dx, dparams = run(net, which, prefix, x, ups, lengths=LENS)
    want_outs, want_dx, want_params = [torch.zeros_like(o) for o in outs], torch.zeros_like(dx), {}
    for b, ln in enumerate(LENS):
        o, g, dp = run(alone, which, prefix, x[b:b + 1, :, :ln].contiguous(), [u[b:b + 1, :, :ln].contiguous() for u in ups])
        for w, t in zip(want_outs, o):
            w[b, :, :ln] = t[0]
        want_dx[b, :, :ln] = g[0]
        for k, t in dp.items():
            want_params[k] = want_params.get(k, 0) + t
    assert set(dparams) == set(want_params) and len(dparams) >= 8

    sel = live.view(2, 1, N, 1)
    pairs = [(f"out{i}", torch.where(sel, o, torch.zeros((), device=DEV)), w, w) for i, (o, w) in enumerate(zip(outs, want_outs))]
    pairs.append(("dx", torch.where(sel, dx, torch.zeros((), device=DEV)), want_dx, want_dx))
    measured_by = ZERO_EXACT.get(which, {})
    for k in sorted(dparams):
        short = k[len(prefix) + 1:]
        pairs.append(("d " + short, dparams[k], want_params[k], want_params[prefix + "." + measured_by.get(short, short)]))
    got_est, want_est = estimates(net, prefix), estimates(alone, prefix)
    moved = 0
    for k in sorted(got_est):
        if k.endswith("num_batches_tracked"):
            assert int(got_est[k]) == int(want_est[k]), k
            moved += int(got_est[k]) > 0
        else:
            pairs.append((k[len(prefix) + 1:], got_est[k], want_est[k], want_est[k]))
    assert moved >= 1

    failures, worst = [], 0.0
    print()
    for name, a, w, by in pairs:
        assert torch.isfinite(a).all(), f"{name}: not finite"
        ratio = float((a.double() - w.double()).abs().max()) / float(by.double().abs().max())
        worst = max(worst, ratio)
        print(f"RATIO {which} {name} max|per sample|={float(w.abs().max()):.3e} scale={float(by.abs().max()):.3e} err/scale={ratio:.3e} of bound={ratio / BOUND:.3f}")
        if not ratio <= BOUND:
            failures.append(f"{name}: {ratio:.2e} of its max-abs, allowed {BOUND:.2e}")

    # the bound must bite: the padded batch without lengths (the padding counted into the statistics and attended to)
    dense, _, _ = run(net, which, prefix, x, ups)
    miss = max(float((torch.where(sel, o, torch.zeros((), device=DEV)).double() - w.double()).abs().max()) / float(w.double().abs().max())
               for o, w in zip(dense, want_outs))
    print(f"RATIO {which} without lengths: outputs miss by {miss / BOUND:.1f} x the bound")
    if not miss > 10 * BOUND:
        failures.append(f"the bound does not see the lengths omitted ({miss / BOUND:.1f} x)")
    assert not failures, "; ".join(failures)


def test_attend_with_lengths_raises_on_the_library_route():
    """Attention dropout at a head width no kernel is built for (24) goes to the library's fused attention, which has no length form."""
    net = hc.build_model(DEV)
    q, kv = torch.randn(2, 8, 48, device=DEV), torch.randn(2, 8, 96, device=DEV)
    with train_forward(net, (0.0, 0.1, 0.0)):
        assert net.attend(q, kv, 2).shape == (2, 8, 48)
        with pytest.raises(RuntimeError, match="lengths"):
            net.attend(q, kv, 2, query_lengths=(8, 5), key_lengths=(8, 5))
