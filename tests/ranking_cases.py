"""Seeded inputs the Hamming-ranking tests share (test_gpu_ranking.py, buffer_contract_cases.py).  No test functions."""
import torch


def spread_codes(Q, N, nbits, seed):
    """Distances of every query spread over (nearly) all bins: row j differs from a base code in j % (nbits + 1) bits,
    queries differ from it in a few more -- the ranking needs several 32-bin windows."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 2, (nbits,), generator=g).float() * 2 - 1
    r = base.repeat(N, 1)
    flips = torch.randint(0, nbits + 1, (N,), generator=g)
    for j in range(N):
        pos = torch.randperm(nbits, generator=g)[:int(flips[j])]
        r[j, pos] *= -1
    q = base.repeat(Q, 1)
    for i in range(Q):
        pos = torch.randperm(nbits, generator=g)[:i % 7]
        q[i, pos] *= -1
    return q, r
