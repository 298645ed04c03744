"""-m "not gpu": the dense and the length-aware entry points of PointConv and of the inference attention share one host path
(csrc/pointconv_tile.h: pc_agg_run, pc_linear_run; csrc/pointconv_grad_tile.h: pcg_run; csrc/attention_forward.h:
attention_forward_run).  Every call below fails validation, so nothing is launched and no device is needed: the dense entry, the
length entry with null lengths and the length entry with aligned lengths must return the same code for the same bad arguments, and
that code is the one the library returned before the host paths were merged (the literals below were recorded from that library)."""
import pytest

from mocopci_amd import _lib

P = 16   # any non-null, 16-byte aligned address
BAD, UNSUPPORTED = 10001, 10002


def forms(dense, lengths):
    """the three forms of one operation as callables of (args before the lengths, args after them)"""
    lib = _lib.load()
    return (lambda a, z: getattr(lib, dense)(*a, *z),
            lambda a, z: getattr(lib, lengths)(*a, None, *z),
            lambda a, z: getattr(lib, lengths)(*a, P, *z))


def agg(b=1, k=32, d=32, s_xyz=P, out=P):
    return (b, 1, 1, d, k, s_xyz, P, P, P), (P, P, P, P, P, P, out, None)


def linear(b=1, k=32, d=32, c_out=32, s_xyz=P, out=P):
    return (b, 1, 1, d, k, s_xyz, P, P, P), (P, P, P, P, P, P, P, c_out, 0.1, out, None)


def agg_grad(b=1, k=32, d=32, s_xyz=P, grad_rows=P, ws=1 << 20):
    return (b, 1, 1, d, k, s_xyz, P, P, P), (P, P, P, P, P, P, P, P, P, grad_rows, P, P, ws, None)


POINTCONV = {
    "mcp_pointconv_agg": (agg, [
        (dict(s_xyz=None), BAD), (dict(b=0), BAD), (dict(k=31), UNSUPPORTED), (dict(out=P + 4), BAD),
        (dict(k=31, out=P + 4), UNSUPPORTED), (dict(b=0, k=31), BAD)]),
    "mcp_pointconv_linear": (linear, [
        (dict(s_xyz=None), BAD), (dict(b=0), BAD), (dict(k=31), UNSUPPORTED), (dict(out=P + 4), BAD),
        (dict(d=32, c_out=64), UNSUPPORTED), (dict(d=32, c_out=64, out=P + 4), UNSUPPORTED)]),
    "mcp_pointconv_agg_grad": (agg_grad, [
        (dict(s_xyz=None), BAD), (dict(b=0), BAD), (dict(k=31), UNSUPPORTED), (dict(grad_rows=P + 4), BAD),
        (dict(d=6), UNSUPPORTED), (dict(ws=0), BAD), (dict(d=6, ws=0), UNSUPPORTED)]),
}


@pytest.mark.parametrize("name", sorted(POINTCONV))
def test_pointconv_forms_reject_the_same_arguments_with_the_same_code(name):
    make, cases = POINTCONV[name]
    calls = forms(name, name + "_lengths")
    for kwargs, want in cases:
        got = [call(*make(**kwargs)) for call in calls]
        assert got == [want] * 3, (name, kwargs, got)


@pytest.mark.parametrize("name", sorted(POINTCONV))
def test_pointconv_lengths_must_be_int32_aligned_and_the_earlier_checks_still_win(name):
    make, _ = POINTCONV[name]
    lengths = getattr(_lib.load(), name + "_lengths")
    call = lambda qlen, **kwargs: (lambda a, z: lengths(*a, qlen, *z))(*make(**kwargs))
    assert call(P + 2) == BAD
    assert call(P + 2, k=31) == UNSUPPORTED      # the shape is checked before any alignment, as it always was
    assert call(P + 2, s_xyz=None) == BAD


def attention(entry, hd=8, stride=None, shift=None, q=P, lens=()):
    lib = _lib.load()
    st = hd if stride is None else stride
    rot = () if shift is None else (shift,)
    return getattr(lib, entry)(2, 1, 1, 1, hd, q, st, P, st, P, st, *rot, 1.0, *lens, P, st, None)


def attention_forms(hd):
    """every entry that takes head width hd without a rotation argument, then the three that take one"""
    fam = "mcp_attention_small" if hd in (8, 16) else "mcp_attention_wide"
    plain = [lambda **kw: attention(fam, hd, **kw)]
    rotated = [lambda shift=0, **kw: attention("mcp_attention", hd, shift=shift, **kw),
               lambda shift=0, **kw: attention("mcp_attention_lengths", hd, shift=shift, lens=(None, None), **kw),
               lambda shift=0, **kw: attention("mcp_attention_lengths", hd, shift=shift, lens=(P, P), **kw)]
    return plain, rotated


@pytest.mark.parametrize("hd", [8, 16, 32, 64, 256])
def test_attention_forms_reject_the_same_arguments_with_the_same_code(hd):
    plain, rotated = attention_forms(hd)
    for call in plain + rotated:
        assert call(stride=hd + 2) == BAD        # float4 rows: strides are multiples of 4 floats
        assert call(q=P + 4) == BAD
        assert call(q=None) == BAD
    for call in rotated:
        assert call(shift=2) == BAD              # kv_batch_shift = bf
        assert call(shift=-1) == BAD
        assert call(shift=2, stride=hd + 2) == BAD


def test_attention_forms_reject_head_width_128():
    for entry, kw in (("mcp_attention_small", {}), ("mcp_attention_wide", {}), ("mcp_attention", dict(shift=0)),
                      ("mcp_attention_lengths", dict(shift=0, lens=(None, None))), ("mcp_attention_lengths", dict(shift=0, lens=(P, P)))):
        assert attention(entry, 128, **kw) == UNSUPPORTED, entry
        assert attention(entry, 128, stride=130, **kw) == UNSUPPORTED, entry   # the width is checked before the strides
    # each narrow / wide entry refuses the other family's widths; mcp_attention takes both
    assert attention("mcp_attention_small", 32) == UNSUPPORTED and attention("mcp_attention_wide", 8) == UNSUPPORTED
    assert attention("mcp_attention_lengths", 8, shift=0, lens=(P + 2, P)) == BAD
    assert attention("mcp_attention_lengths", 128, shift=0, lens=(P + 2, P)) == UNSUPPORTED
