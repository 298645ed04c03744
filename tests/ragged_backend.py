"""TEST INFRASTRUCTURE: the CPU reference of the ragged forward.  A subclass of oracle.backend.OracleBackend whose length-taking
methods do what the definition says -- element b is the cloud x[b, :len[b]] alone --: they run the parent on the live prefix of
every element and pad the result with zeros.  Installed with mocopci_amd.ops.set_backend(RaggedBackend()); inference only (the
train-mode fusion layer has no reference here)."""
import torch

from oracle.backend import OracleBackend


def _lens(lengths, batch, limit):
    if lengths is None:
        return [limit] * batch
    return [min(max(int(v), 0), limit) for v in torch.as_tensor(lengths).reshape(-1).tolist()]


def _per_element(batch, fn, shape, dtype):
    """fn(b) -> (rows_b, ...) for the live prefix of element b (None: no live row); zero-padded to (batch, *shape)."""
    out = torch.zeros((batch, *shape), dtype=dtype)
    for b in range(batch):
        r = fn(b)
        if r is not None:
            out[b, :r.shape[0]] = r
    return out


class RaggedBackend(OracleBackend):
    name = "oracle-cpu-ragged"

    def fps(self, xyz, npoint, with_points=False, lengths=None):
        if lengths is None:
            return super().fps(xyz, npoint, with_points=with_points)
        B, N, _ = xyz.shape
        ls = _lens(lengths, B, N)
        sel = _per_element(B, lambda b: super(RaggedBackend, self).fps(xyz[b:b + 1, :ls[b]].contiguous(), npoint)[0] if ls[b] else None, (npoint,),
                           torch.int32)
        return (sel, self.group_rows(xyz, sel)) if with_points else sel

    def knn(self, query, ref, k, mode=0, return_dist=False, query_lengths=None, ref_lengths=None):
        if query_lengths is None and ref_lengths is None:
            return super().knn(query, ref, k, mode=mode, return_dist=return_dist)
        assert not return_dist
        B, Q, _ = query.shape
        ql, rl = _lens(query_lengths, B, Q), _lens(ref_lengths, B, ref.shape[1])

        def one(b):
            if not ql[b] or not rl[b]:
                return None
            kk = min(k, rl[b])
            idx = super(RaggedBackend, self).knn(query[b:b + 1, :ql[b]].contiguous(), ref[b:b + 1, :rl[b]].contiguous(), kk, mode=mode)[0]
            return idx if kk == k else torch.cat([idx, idx[:, -1:].expand(-1, k - kk)], dim=1)   # fewer references than k: the last live entry again
        return _per_element(B, one, (Q, k), torch.int32)

    def pointconv_agg(self, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, centre_lengths=None):
        if centre_lengths is None:
            return super().pointconv_agg(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2)
        B, S, _ = new_xyz.shape
        ls = _lens(centre_lengths, B, S)
        one = lambda b: super(RaggedBackend, self).pointconv_agg(s_xyz[b:b + 1], new_xyz[b:b + 1, :ls[b]], s_points[b:b + 1], idx[b:b + 1, :ls[b]],
                                                                 w0, b0, w1, b1, w2, b2)[0] if ls[b] else None
        return _per_element(B, one, (S, (s_points.shape[-1] + 3) * 8), torch.float32)

    def pointconv_linear(self, s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, w, b, slope, packed=None, centre_lengths=None):
        if centre_lengths is None:
            return super().pointconv_linear(s_xyz, new_xyz, s_points, idx, w0, b0, w1, b1, w2, b2, w, b, slope, packed=packed)
        B, S, _ = new_xyz.shape
        ls = _lens(centre_lengths, B, S)
        one = lambda bb: super(RaggedBackend, self).pointconv_linear(s_xyz[bb:bb + 1], new_xyz[bb:bb + 1, :ls[bb]], s_points[bb:bb + 1],
                                                                     idx[bb:bb + 1, :ls[bb]], w0, b0, w1, b1, w2, b2, w, b, slope)[0] if ls[bb] else None
        return _per_element(B, one, (S, w.shape[0]), torch.float32)

    def fusion_mlp(self, p1, p2, idx, w1, b1, w2, b2, w3, b3, lengths=None):
        if lengths is None:
            return super().fusion_mlp(p1, p2, idx, w1, b1, w2, b2, w3, b3)
        idx = torch.cat(list(idx), dim=-1) if isinstance(idx, (tuple, list)) else idx
        B, N, _ = p1.shape
        ls = _lens(lengths, B, N)
        one = lambda b: super(RaggedBackend, self).fusion_mlp(p1[b:b + 1, :ls[b]], p2[b:b + 1], idx[b:b + 1, :ls[b]], w1, b1, w2, b2, w3, b3)[0] \
            if ls[b] else None
        return _per_element(B, one, (N, 3), torch.float32)

    def fusion_bn(self, *a, **k):
        raise NotImplementedError("the ragged CPU reference is inference only")
