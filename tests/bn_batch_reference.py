"""Float64 statement of BatchNorm on batch statistics with per-group lengths (csrc/bn_batch.hip; include/mocopci_hip.h:
mcp_bn_batch_forward / mcp_bn_batch_backward), forward and backward, and the cases of test_bn_batch_gpu.py.  A plain module:
test_bn_batch_cpu.py checks it against torch.nn.functional.batch_norm(training=True) on every group cut to its length.

x is (G, F, N, C); row (f, i) of group g is live iff i < lens[g], m_g = F * lens[g].  Per group and channel, over the live rows:
mean, the biased variance, y = (x - mean) * gamma * rsqrt(var + eps) + beta, and for an upstream gradient dy
dx = gamma * rstd * (dy - sum(dy) / m - xhat * sum(dy * xhat) / m); dgamma / dbeta sum dy * xhat / dy over all groups' live rows.
m = 0: mean 0, var 0; padded rows of y and dx are zero."""
from types import SimpleNamespace

import torch

EPS = 1e-5
# csrc/bn_batch.hip cuts a group's F * N rows into chunks (parts) of at least 256 rows: 3 * 256 rows are exactly 3 parts of 256 rows
# (test_bn_batch_cpu.py asserts it through mcp_bn_batch_parts), so with F = 1 a length below 512 leaves the third part entirely padded
PART_ROWS = 256
N_PARTS = 3 * PART_ROWS

# tag: the edge the case reaches
CASES = [
    dict(tag="one-row", g=1, f=1, n=5, c=64, lens=(1,)),                                  # m = 1: var 0
    dict(tag="none-live", g=2, f=2, n=7, c=32, lens=(0, 0)),                              # m = 0 everywhere
    dict(tag="empty-middle", g=3, f=5, n=37, c=64, lens=(37, 0, 11)),
    dict(tag="frames", g=2, f=5, n=100, c=128, lens=(100, 63)),                           # live rows are not contiguous across frames
    dict(tag="wide", g=2, f=2, n=130, c=256, lens=(129, 1)),
    dict(tag="parts-tail", g=2, f=1, n=N_PARTS, c=64, lens=(PART_ROWS + 44, N_PARTS)),    # a length ends inside part 1: part 2 is all padding
    dict(tag="parts-boundary", g=2, f=1, n=N_PARTS, c=64, lens=(2 * PART_ROWS, PART_ROWS)),   # lengths exactly on part boundaries
    dict(tag="far", g=2, f=2, n=64, c=64, lens=(64, 32), far=True),                       # half the channels 300 + 0.1 randn
]


def case_id(c):
    return f"bn_batch[{c['tag']},g={c['g']},f={c['f']},n={c['n']},c={c['c']},lens={'-'.join(str(v) for v in c['lens'])}]"


def live_rows(case):
    """(G, N) bool"""
    return torch.arange(case["n"]).view(1, -1) < torch.tensor(case["lens"]).view(-1, 1)


def forward(x, lens, gamma, beta, eps=EPS, skip=None):
    """x (G,F,N,C) float64 -> (y, mean (G,C), var (G,C), count (G)).  skip: (g, flat live row) left out of that group's statistics
    (the mutants of the GPU test)."""
    G, Fr, N, C = x.shape
    y = torch.zeros_like(x)
    mean, var = x.new_zeros((G, C)), x.new_zeros((G, C))
    count = torch.zeros((G,), dtype=torch.int64)
    for g in range(G):
        ln = int(lens[g])
        rows = x[g, :, :ln].reshape(-1, C)
        count[g] = rows.shape[0]
        if skip is not None and skip[0] == g:
            keep = torch.ones(rows.shape[0], dtype=torch.bool)
            keep[skip[1]] = False
            rows = rows[keep]
        if rows.shape[0] == 0:
            continue
        mean[g] = rows.mean(dim=0)
        var[g] = (rows - mean[g]).square().mean(dim=0)
        y[g, :, :ln] = (x[g, :, :ln] - mean[g]) * (gamma * torch.rsqrt(var[g] + eps)) + beta
    return y, mean, var, count


def backward(x, lens, gamma, mean, var, dy, eps=EPS, skip=None):
    """-> (dx, dgamma, dbeta).  skip: (g, flat live row) whose term is left out of dgamma / dbeta (the affine mutant)."""
    G, Fr, N, C = x.shape
    dx = torch.zeros_like(x)
    dgamma, dbeta = x.new_zeros((C,)), x.new_zeros((C,))
    for g in range(G):
        ln = int(lens[g])
        m = Fr * ln
        if m == 0:
            continue
        rstd = torch.rsqrt(var[g] + eps)
        xhat = (x[g, :, :ln] - mean[g]) * rstd
        d = dy[g, :, :ln]
        s1, s2 = d.sum(dim=(0, 1)), (d * xhat).sum(dim=(0, 1))
        dx[g, :, :ln] = gamma * rstd * (d - s1 / m - xhat * s2 / m)
        if skip is not None and skip[0] == g:
            s1 = s1 - d.reshape(-1, C)[skip[1]]
            s2 = s2 - (d * xhat).reshape(-1, C)[skip[1]]
        dgamma += s2
        dbeta += s1
    return dx, dgamma, dbeta


_PREPARED = {}


def prepare(case):
    """The case's float32 inputs (CPU) and the float64 results, computed once and shared: x, dy, gamma, beta, live (G,N) and ev with
    y, mean, var, count, dx, dgamma, dbeta."""
    key = case["tag"]
    if key not in _PREPARED:
        G, Fr, N, C = case["g"], case["f"], case["n"], case["c"]
        gen = torch.Generator().manual_seed(1000 + len(key) + 7 * C + N)
        x = torch.randn(G, Fr, N, C, generator=gen) * (0.5 + torch.rand(C, generator=gen)) + torch.randn(C, generator=gen)
        if case.get("far"):
            x[..., C // 2:] = 300.0 + 0.1 * torch.randn(G, Fr, N, C - C // 2, generator=gen)
        dy = torch.randn(G, Fr, N, C, generator=gen)
        gamma = 1.0 + 0.3 * torch.randn(C, generator=gen)
        beta = 0.2 * torch.randn(C, generator=gen)
        lens = torch.tensor(case["lens"])
        y, mean, var, count = forward(x.double(), lens, gamma.double(), beta.double())
        dx, dgamma, dbeta = backward(x.double(), lens, gamma.double(), mean, var, dy.double())
        ev = SimpleNamespace(y=y, mean=mean, var=var, count=count, dx=dx, dgamma=dgamma, dbeta=dbeta)
        _PREPARED[key] = SimpleNamespace(case=case, x=x, dy=dy, gamma=gamma, beta=beta, lens=lens, live=live_rows(case), ev=ev)
    return _PREPARED[key]
