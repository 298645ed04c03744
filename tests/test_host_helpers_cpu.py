"""-m "not gpu": the two host helpers of mocopci_amd/ops.py whose behaviour callers rely on without a kernel in between."""
import torch

from mocopci_amd import ops


def test_split_flat_returns_views_in_order_that_cover_the_buffer():
    like = [torch.empty(3, 4), torch.empty(3), torch.empty(2, 3, 1), torch.empty(0), torch.empty(())]
    buf = torch.arange(sum(t.numel() for t in like), dtype=torch.float32)
    pieces = ops._split_flat(buf, like)
    assert [p.shape for p in pieces] == [t.shape for t in like]
    at = 0
    for p in pieces:   # each piece is a view of the buffer at the running offset: same storage, consecutive, nothing copied
        assert p.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() and p.storage_offset() == at and p.is_contiguous()
        at += p.numel()
    assert at == buf.numel()
    assert torch.equal(torch.cat([p.reshape(-1) for p in pieces]), buf)
    pieces[1].fill_(-1.0)
    assert torch.equal(buf[12:15], torch.full((3,), -1.0))


def test_route_predicates_read_their_table_at_call_time(monkeypatch):
    assert not ops._routes({}, "a", 10 ** 9)
    assert ops._routes({"a": 5}, "a", 5) and not ops._routes({"a": 5}, "a", 4) and not ops._routes({"a": 5}, "b", 5)
    cls = ops.fp_mlp_class(64, 3, (64, 64))
    for table, predicate in (("FP_MLP_FUSED_CLASSES", ops.fp_mlp_routes_fused), ("FP_MLP_GRAD_FUSED_CLASSES", ops.fp_mlp_grad_routes_fused),
                             ("FP_MLP_BN_FUSED_CLASSES", ops.fp_mlp_bn_routes_fused)):
        monkeypatch.setattr(ops, table, {})
        assert not predicate(64, 3, (64, 64), 1 << 20)
        monkeypatch.setattr(ops, table, {cls: 128})
        assert predicate(64, 3, (64, 64), 128) and not predicate(64, 3, (64, 64), 127)
    cls = ops.group_mlp_class(4, (32, 32, 64), 16)
    for table, predicate in (("GROUP_MLP_FUSED_CLASSES", ops.group_mlp_routes_fused), ("GROUP_MLP_GRAD_FUSED_CLASSES", ops.group_mlp_grad_routes_fused),
                             ("GROUP_MLP_BN_FUSED_CLASSES", ops.group_mlp_bn_routes_fused)):
        monkeypatch.setattr(ops, table, {cls: 128})
        assert predicate(4, (32, 32, 64), 16, 128) and not predicate(4, (32, 32, 64), 16, 127) and not predicate(4, (32, 32, 64), 64, 128)
