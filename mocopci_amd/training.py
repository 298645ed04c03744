"""The reference's training objective (train.py:135-160) on the outputs of MoCoPCI.forward(train=True)."""
from . import ops

ALPHA = (1.0, 0.8, 0.4, 0.2)  # train.py:138


def chamfer_loss(pred, gt, rows=None, gt_lengths=None):
    """models/utils.py:36-45 on the layouts train.py uses: pred (B,n,3) (the reference permutes its (B,n,3) frame to (B,3,n) and
    chamfer_loss permutes it back), gt (B,3,n).  rows: a memo {id(gt): (gt, its (B,n,3) copy)} so that a ground-truth cloud compared
    with several predictions is laid out once (and, inside a cloud_scope, sorted for the neighbour searches once).  The entry holds
    gt itself: a temporary view (zip over a stacked tensor) would otherwise die and hand its id to the next frame's view.
    gt_lengths: per-sample point counts of a zero-padded ground truth, passed through as the Chamfer distance's y_lengths (only the
    first gt_lengths[b] points of gt[b] count; ops.HipBackend.chamfer)."""
    if rows is None:
        g = gt.transpose(1, 2).contiguous()
    else:
        hit = rows.get(id(gt))
        if hit is None or hit[0] is not gt:
            hit = rows[id(gt)] = (gt, gt.transpose(1, 2).contiguous())
        g = hit[1]
    if gt_lengths is not None:
        return ops.backend().chamfer(pred.contiguous(), g, y_lengths=gt_lengths)
    return ops.backend().chamfer(pred.contiguous(), g)


def emd_loss(pred, gt, gt_lengths=None):
    """models/utils.py:223-235 (EMD) on chamfer_loss's layouts: pred (B,n,3), gt (B,3,n) -> mean over the batch of cost / n,
    differentiable.  gt_lengths: per-sample point counts of a zero-padded ground truth, passed through as the EMD's lengths2."""
    from . import emd
    return emd.EMD(pred.transpose(1, 2), gt, lengths2=gt_lengths)


def multiscale_loss(frames_lst_f, frames_lst_b, gt_frame, out_lst, gt, lengths1=None, lengths2=None, gt_lengths=None):
    """losssum of train.py:135-160: final frames vs gt, the two full-resolution warps of both directions, and the level 1..3
    frames against the FPS-downsampled ground truth with weights alpha[1:].  The 33 Chamfer terms share 12 ground-truth clouds;
    terms that compare several predictions with the SAME cloud are evaluated as one call on a stacked batch (per-sample values,
    then the reference's sums): 15 calls, 30 searches, instead of 33 / 66 -- the same terms, added in the reference's order.
    lengths1 / lengths2 / gt_lengths (three (B,) lengths): the lengths the forward was given (MoCoPCI.forward).  The level-0 terms
    -- the final frames and the four full-resolution warps per triple -- then pass x_lengths / y_lengths to their Chamfer calls:
    frames 0, 1 are live below l1, frame 2 below l2, the two mixed warps below min(l1, l2), the ground truth below gt_lengths[i]
    (None: full).  The sampled levels are full."""
    with ops.backend().cloud_scope():
        return _multiscale_loss(frames_lst_f, frames_lst_b, gt_frame, out_lst, gt, _level0_lengths(out_lst, lengths1, lengths2, gt_lengths))


def _level0_lengths(out_lst, lengths1, lengths2, gt_lengths):
    """{"out": per frame, "f": (l1, min), "b": (l2, min), "gt": per frame} as (B,) device arrays, or None without lengths."""
    if lengths1 is None and lengths2 is None and gt_lengths is None:
        return None
    import torch
    B, N, dev = out_lst[0].shape[0], out_lst[0].shape[1], out_lst[0].device
    one = lambda l: torch.full((B,), N, dtype=torch.int32, device=dev) if l is None else ops.lengths_tensor(l, B, N, dev).to(dev)
    l1, l2 = one(lengths1), one(lengths2)
    both = torch.minimum(l1, l2)
    if gt_lengths is not None and len(gt_lengths) != len(out_lst):
        raise RuntimeError(f"gt_lengths: expected {len(out_lst)} (B,) lengths, got {len(gt_lengths)}")
    return {"out": (l1, l1, l2), "f": (l1, both), "b": (l2, both), "gt": [None] * len(out_lst) if gt_lengths is None else list(gt_lengths)}


def _stacked(preds, gt_rows, x_lengths=None, y_lengths=None):
    """Chamfer of every prediction in `preds` (each (B,n,3)) against the same ground-truth cloud (B,m,3): a (len(preds),) tensor, the
    mean over B per prediction -- one call on the stacked batch.  x_lengths: one (B,) array per prediction; y_lengths: the ground
    truth's (or None: full)."""
    import torch
    B = preds[0].shape[0]
    if x_lengths is not None:
        M = gt_rows.shape[1]
        yl = None if y_lengths is None else ops.lengths_tensor(y_lengths, B, M, gt_rows.device).to(gt_rows.device).repeat(len(preds))
        v = ops.backend().chamfer(torch.cat([p.contiguous() for p in preds], dim=0), gt_rows.repeat(len(preds), 1, 1), per_sample=True,
                                  x_lengths=torch.cat(list(x_lengths)), y_lengths=yl)
        return v.reshape(len(preds), B).mean(dim=1)
    if len(preds) == 1:
        return ops.backend().chamfer(preds[0].contiguous(), gt_rows).reshape(1)
    v = ops.backend().chamfer(torch.cat([p.contiguous() for p in preds], dim=0), gt_rows.repeat(len(preds), 1, 1), per_sample=True)
    return v.reshape(len(preds), B).mean(dim=1)   # one mean (backward: one expand), not a slice per term


_weights = {}   # (signature, device) -> (total weights (T,), part weights (5,T)) on the device, built once


def _multiscale_loss(frames_lst_f, frames_lst_b, gt_frame, out_lst, gt, lens=None):
    """The terms as ONE vector t (in the order below) and the objective as one dot product with a constant weight vector -- the
    reference's nested sums (train.py:135-160) are 70 scalar adds and multiplies, each an autograd node with a launch of its own:
        final      sum of the terms of out_lst                                  weight 1     in the total
        straight   0.5 (f0 + f1) per triple, forward and backward               weight 1/2
        multi      ALPHA[l+1] x term per triple and level, forward and backward weight 1/4"""
    import torch
    rows = lambda g: g.transpose(1, 2).contiguous()   # (B,3,n) as train.py holds the ground truth -> (B,n,3)
    vals, spec = [], []                               # spec: (part index, weight inside the part) per term
    for i, (frames, g) in enumerate(zip(out_lst, gt)):
        vals.append(_stacked([frames], rows(g)) if lens is None else _stacked([frames], rows(g), [lens["out"][i]], lens["gt"][i]))
        spec.append((0, 1.0))
    for i, (frames_f, frames_b, gts) in enumerate(zip(frames_lst_f, frames_lst_b, gt_frame)):
        level0 = [frames_f[0], frames_f[1], frames_b[0], frames_b[1]]
        vals.append(_stacked(level0, rows(gts[0])) if lens is None else _stacked(level0, rows(gts[0]), [*lens["f"], *lens["b"]], lens["gt"][i]))
        spec += [(1, 0.5), (1, 0.5), (2, 0.5), (2, 0.5)]
        for l in range(len(ALPHA) - 1):
            vals.append(_stacked([frames_f[l + 2], frames_b[l + 2]], rows(gts[l + 1])))
            spec += [(3, ALPHA[l + 1]), (4, ALPHA[l + 1])]
    t = torch.cat(vals)
    key = (tuple(spec), str(t.device))
    if key not in _weights:
        in_total = (1.0, 0.5, 0.5, 0.25, 0.25)        # final, straight_f, straight_b, multi_f, multi_b
        parts_w = torch.zeros(5, len(spec))
        for i, (k, w) in enumerate(spec):
            parts_w[k, i] = w
        total_w = (torch.tensor(in_total).unsqueeze(1) * parts_w).sum(0)
        _weights[key] = (total_w.to(t.device), parts_w.to(t.device))
    total_w, parts_w = _weights[key]
    total = torch.dot(t, total_w)
    parts = parts_w @ t.detach()
    return total, {"final": parts[0], "straight_f": parts[1], "straight_b": parts[2], "multi_f": parts[3], "multi_b": parts[4]}


def train_step(net, optimizer, xyz1, xyz2, gt, clip=2.0, lengths1=None, lengths2=None, gt_lengths=None):
    """One iteration of train.py:123-167: forward, loss, backward, gradient-norm clipping at 2.0, optimizer step.
    lengths1 / lengths2 / gt_lengths: a padded batch (MoCoPCI.forward, multiscale_loss)."""
    import torch
    if lengths1 is None and lengths2 is None and gt_lengths is None:
        frames_f, frames_b, gt_frame, out_lst = net(xyz1, xyz2, gt, None, True)
        loss, parts = multiscale_loss(frames_f, frames_b, gt_frame, out_lst, gt)
    else:
        frames_f, frames_b, gt_frame, out_lst = net(xyz1, xyz2, gt, None, True, lengths1=lengths1, lengths2=lengths2, gt_lengths=gt_lengths)
        loss, parts = multiscale_loss(frames_f, frames_b, gt_frame, out_lst, gt, lengths1, lengths2, gt_lengths)
    optimizer.zero_grad()
    with ops.segments_memo():
        loss.backward()
    torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
    optimizer.step()
    return float(loss.detach()), {k: float(v.detach()) for k, v in parts.items()}
