"""NL-Drive data path, same on-disk format and sampling rule as the reference's
data/no_norm_datasets.py:8-91:

  * a frame is a flat little-endian float32 file of xyz triples (np.fromfile(...).reshape(-1, 3), :47);
  * a scene list has one sequence per line: 4 input frame names (frames 01,05,09,13) followed by the
    ground-truth frames (06,07,08), space separated (:26-33);
  * every frame is resampled to num_points: a random subset without replacement when it has enough points,
    otherwise all points followed by a random fill WITH replacement (:52-55) -- which is where the exact
    duplicate points in the inputs come from;
  * __getitem__ -> (input: num_frames x (N,3) tensors, gt: (interval-1) x (N,3) tensors).
np.random is used in the reference's call order, so a seeded run reproduces the reference's sample.

GPU-side resampling (NLDriveDataset(device=...)): the raw scan is uploaded once, whole, and the row selection runs on the GPU
(mcp_group_rows); the index list still comes from np.random in the reference's call order (O(N) host work, no point data
touched on the host), so the sample is bit-identical to the host path's and the duplicated rows are exact duplicates.

Whole ground-truth frames (NLDriveDataset(raw_gt=True)): the ground-truth scans come back as recorded, every one with its own
point count, and no random draw is made for them; collate_padded() zero-pads them per batch and returns the counts, and
evaluate(raw_gt=True) hands those to the Chamfer distance as y_lengths -- the metric against the scan itself instead of against a
random num_points subsample of it.  The inputs' draws come first in the reference's call order, so the inputs do not change.
evaluate(raw_gt=True, raw_emd=True) reports the EMD the same way: emd.EMD(lengths2=) runs the auction on each scan's own points.
evaluate(raw_gt=True, gt_points=K) first reduces every whole scan to at most K points by furthest point sampling on the GPU
(downsample_padded: one launch of the length-aware sampler per frame): a deterministic, coverage-preserving subset instead of a
random draw, and a bounded size for the auction.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset


def read_frame(path):
    return np.fromfile(path, dtype=np.float32, count=-1).reshape([-1, 3])


def write_frame(path, xyz):
    np.asarray(xyz, dtype=np.float32).reshape(-1, 3).tofile(path)


def resample_indices(num, num_points):
    if num >= num_points:
        return np.random.choice(num, num_points, replace=False)
    return np.concatenate((np.arange(num), np.random.choice(num, num_points - num, replace=True)), axis=-1)


def resample_on_device(raw, pick, device):
    """raw (n,3) float32 numpy scan, pick (num_points,) indices -> (num_points,3) float32 tensor on `device`, gathered there."""
    from . import ops
    pts = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).to(device, non_blocking=True).unsqueeze(0)
    idx = torch.from_numpy(np.ascontiguousarray(pick, dtype=np.int32)).to(device, non_blocking=True).unsqueeze(0)
    return ops.backend().group_rows(pts, idx)[0]


class NLDriveDataset(Dataset):
    def __init__(self, data_root, scene_list, num_points=8192, interval=4, num_frames=4, device=None, raw_gt=False):
        """device: None = the reference's host path (numpy fancy indexing); a CUDA device = GPU-side resampling (use with
        num_workers=0: the frames come back as tensors of that device).  raw_gt: the ground-truth frames whole, (n_j,3) each with
        its own n_j, instead of resampled to num_points (batch them with collate_padded)."""
        super().__init__()
        self.device = device
        self.raw_gt = raw_gt
        self.data_root, self.scene_list = data_root, scene_list
        self.num_points, self.interval, self.num_frames = num_points, interval, num_frames
        with open(scene_list, "r") as fh:
            self.velodynes = [line.strip("\n").split(" ") for line in fh.readlines()]

    def __len__(self):
        return len(self.velodynes)

    def __getitem__(self, index):
        names = self.velodynes[index]
        frames, picks = [], []
        for i in range(self.num_frames):
            raw = read_frame(os.path.join(self.data_root, names[i]))
            frames.append(raw)
            picks.append(resample_indices(raw.shape[0], self.num_points))
        num_gt = len(names) - self.num_frames
        gt_intv = num_gt // (self.interval - 1)
        gts, gpicks = [], []
        for i in range(self.interval - 1):
            raw = read_frame(os.path.join(self.data_root, names[3 + (i + 1) * gt_intv]))
            gts.append(raw)
            if not self.raw_gt:
                gpicks.append(resample_indices(raw.shape[0], self.num_points))
        if self.raw_gt:
            whole = [torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)) for f in gts]
            if self.device is not None:
                return ([resample_on_device(f, p, self.device) for f, p in zip(frames, picks)],
                        [t.to(self.device, non_blocking=True) for t in whole])
            return [torch.from_numpy(f[p, :].astype("float32")) for f, p in zip(frames, picks)], whole
        if self.device is not None:
            return ([resample_on_device(f, p, self.device) for f, p in zip(frames, picks)],
                    [resample_on_device(f, p, self.device) for f, p in zip(gts, gpicks)])
        inp = [torch.from_numpy(f[p, :].astype("float32")) for f, p in zip(frames, picks)]
        gt = [torch.from_numpy(f[p, :].astype("float32")) for f, p in zip(gts, gpicks)]
        return inp, gt


def collate_padded(batch):
    """collate_fn for NLDriveDataset(raw_gt=True): batch = [(inputs, gts), ...] -> (inputs, gts, gt_lengths).  inputs: num_frames
    stacked (B,N,3) tensors, as the default collate gives.  gts[j] (B, L_j, 3): frame j of every sample, zero-padded to the longest
    one of the batch (L_j >= 1); gt_lengths[j] (B,) int32 on the CPU: the point counts, the y_lengths of the Chamfer distance."""
    inputs = [torch.stack([item[0][i] for item in batch]) for i in range(len(batch[0][0]))]
    gts, lengths = [], []
    for j in range(len(batch[0][1])):
        frames = [item[1][j] for item in batch]
        out = frames[0].new_zeros((len(frames), max(1, max(f.shape[0] for f in frames)), 3))
        for b, f in enumerate(frames):
            out[b, :f.shape[0]] = f
        gts.append(out)
        lengths.append(torch.tensor([f.shape[0] for f in frames], dtype=torch.int32))
    return inputs, gts, lengths


def downsample_padded(clouds, lengths, num_points):
    """A padded batch reduced to at most num_points points per cloud by furthest point sampling: clouds (B,L,3) on the GPU,
    lengths (B,) (forms: ops.lengths_tensor) -> (points (B,num_points,3), new_lengths (B,) int32 on the clouds' device) with
    new_lengths = min(lengths, num_points).  Row j < new_lengths[b] is the j-th furthest-point sample of clouds[b, :lengths[b]]
    (start point: row 0; a cloud shorter than num_points comes back whole, in sampling order); rows at or beyond the new length are
    zero.  One launch of the length-aware sampler with its coordinate output; padded rows of `clouds` are never read."""
    from . import ops
    clouds = clouds.contiguous()
    B, L = clouds.shape[0], clouds.shape[1]
    lens = ops.lengths_tensor(lengths, B, L, clouds.device)
    _, points = ops.backend().fps(clouds, num_points, with_points=True, lengths=lens)
    new_lengths = lens.clamp(0, min(L, num_points))
    pad = torch.arange(num_points, device=clouds.device).view(1, num_points) >= new_lengths.view(B, 1)
    return points.masked_fill(pad.unsqueeze(-1), 0.0), new_lengths


def evaluate(net, loader, device="cuda", raw_gt=False, raw_emd=False, gt_points=None):
    """The evaluation loop of test.py:71-135 in its intended form (one forward -> 3 frames; test.py:84 passes
    train=True by mistake): per-frame Chamfer distance and EMD means, forward time with device sync.
    raw_gt: the loader yields collate_padded batches of NLDriveDataset(raw_gt=True); the Chamfer distance is taken against the
    whole ground-truth scans (y_lengths = their point counts).  "emd" is None unless raw_emd is set too: then it holds the per-frame
    means of EMD(out_j, gt_j, lengths2 = the scans' point counts), the auction between the prediction and each whole scan.
    raw_emd has a meaning only together with raw_gt: without raw_gt the ground truth is already resampled to full clouds, the EMD is
    always reported and raw_emd is ignored.
    gt_points (with raw_gt): every whole scan is first reduced to at most gt_points points by downsample_padded (furthest point
    sampling on the GPU), and the new point counts are the y_lengths / lengths2 of the two metrics.  None: the scans as they are."""
    import time

    from . import emd as emd_mod, ops
    cd = [[], [], []]
    emd = [[], [], []]
    seconds = []
    with torch.no_grad():
        for sample in loader:
            inp, gt = sample[0], sample[1]
            inp = [t.permute(0, 2, 1).to(device).contiguous().float() for t in inp]   # (B,3,N), test.py:73-74
            gt = [t.to(device).contiguous().float() for t in gt]                      # (B,N,3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = net(inp[1], inp[2])                                                  # the two middle frames, test.py:84
            torch.cuda.synchronize()
            seconds.append(time.perf_counter() - t0)
            with ops.backend().cloud_scope():   # a cloud the metrics search in both roles is sorted once per batch
                for j in range(3):
                    if raw_gt:
                        scan, count = gt[j], sample[2][j]
                        if gt_points is not None:
                            scan, count = downsample_padded(scan, count, gt_points)
                        cd[j].append(float(ops.backend().chamfer(out[j].contiguous(), scan, y_lengths=count)))
                        if raw_emd:
                            emd[j].append(float(emd_mod.EMD(out[j].permute(0, 2, 1).contiguous(), scan.permute(0, 2, 1).contiguous(),
                                                            lengths2=count)))
                        continue
                    cd[j].append(float(ops.backend().chamfer(out[j].contiguous(), gt[j])))
                    emd[j].append(float(emd_mod.EMD(out[j].permute(0, 2, 1).contiguous(), gt[j].permute(0, 2, 1).contiguous())))
    mean = lambda v: float(np.mean(v)) if v else float("nan")
    with_emd = raw_emd or not raw_gt
    return {"chamfer": [mean(c) for c in cd], "emd": [mean(e) for e in emd] if with_emd else None, "seconds_per_forward": mean(seconds),
            "sequences": len(loader.dataset)}
