"""Shared by tests/test_ip_map_host.py and tests/test_gpu_ip_map.py: seeded inputs of wv_ip_map_at_k and their references.
No test functions.  Everything is made on the host, once per case (functools caches), and never modified.

Embeddings
  grid   round(tanh(randn) * 256) / 256 with D <= 128: every product is a multiple of 2^-16 and every partial sum is <= 128,
         so fp32 is exact in ANY summation order, and so is the reference's key 0.5 * (D - s).  On these inputs
         oracle.ranking.calculate_maphashing(..., stable=True) is the reference's own arithmetic with this project's tie rule
         (descending score = ascending key, ties by ascending row): no rounding ambiguity.
  ties   values in {-1, -0.75, ..., 1}: exact like the grid, and many equal scores.
  raw    unrounded randn: for kernel-against-twin and twin-against-composition equality only (no oracle).
  pm1    +-1 codes: the inner-product order is the Hamming order.
  equal  every database row the same vector: every score equal, positions follow row order.
Labels: multi-hot Bernoulli, (classes, p) = (20, 0.07) / (38, 0.10) for one label word, (80, 0.036) for two; some rows carry
no tag.  `word2`: the (80, 0.036) labels with classes 0..63 cleared -- hits lie in the second label word only.
"""
import collections
import functools

import torch

from oracle import ranking

AP_TOL = 1e-6            # what the wrapper tests hold wv_map_at_k to against the oracle's per-query AP
LABELS = {1: (38, 0.10), 2: (80, 0.036)}
SMALL_LABELS = (20, 0.07)

Case = collections.namedtuple("Case", "Q N D lwords k kind seed")
Inputs = collections.namedtuple("Inputs", "q db ql rl qlp rlp k")


def grid_embeddings(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.tanh(torch.randn(n, D, generator=g)) * 256) / 256


def tie_embeddings(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 9, (n, D), generator=g).float() / 4 - 1


def raw_embeddings(n, D, seed):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def pm1_codes(n, D, seed):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed))
    return torch.where(x >= 0, torch.ones_like(x), -torch.ones_like(x))


def multi_hot(n, classes, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, classes, generator=g) < p).float()


def pack_bits(x):
    """[rows, n] (> 0 = set) -> int64 [rows, ceil(n / 64)], bit j of word w = x[:, 64 w + j]: what pack_labels makes"""
    rows, n = x.shape
    words = (n + 63) // 64
    b = torch.zeros((rows, words * 64), dtype=torch.int64)
    b[:, :n] = (x > 0).long()
    return (b.view(rows, words, 64) << torch.arange(64, dtype=torch.int64)).sum(2)


_EMBED = {"grid": grid_embeddings, "ties": tie_embeddings, "raw": raw_embeddings, "pm1": pm1_codes, "word2": grid_embeddings}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The tensors of a case (host, fp32 / int64): never modified by a test."""
    c = case
    classes, p = LABELS[c.lwords] if c.N > 65 or c.lwords == 2 else SMALL_LABELS
    if c.kind == "equal":
        q = grid_embeddings(c.Q, c.D, c.seed)
        db = grid_embeddings(1, c.D, c.seed + 1).expand(c.N, c.D).contiguous()
    else:
        q, db = _EMBED[c.kind](c.Q, c.D, c.seed), _EMBED[c.kind](c.N, c.D, c.seed + 1)
    ql, rl = multi_hot(c.Q, classes, p, c.seed + 2), multi_hot(c.N, classes, p, c.seed + 3)
    if c.kind == "word2":
        ql[:, :64] = 0
        rl[:, :64] = 0
        ql[0, 64:] = rl[:, 64:].amax(0)                     # one query that is sure to hit (in the second word)
    if c.kind == "equal":
        ql[-1] = 0                                          # a query without a hit
        ql[0] = rl.amax(0)                                  # ... and one that hits every tagged row
    return Inputs(q, db, ql, rl, pack_bits(ql), pack_bits(rl), c.k)


@functools.lru_cache(maxsize=None)
def oracle_ap(case):
    """(per-query AP float64 [Q], hits int32 [Q]) of the oracle on an EXACT case (grid, ties, pm1, equal, word2)."""
    assert case.kind != "raw" and case.D <= 128
    x = inputs(case)
    if case.N == 1:       # the oracle, like the reference, squeezes a one-row ranking to a scalar and cannot index it:
        rel = ranking.label_comparison_fn(x.ql, x.rl)[:, 0]       # the only row is at rank 1, AP = 1 if it shares a tag
        return rel.double(), rel.int()
    _, per_query = ranking.calculate_maphashing(x.q, x.ql, x.db, x.rl, x.k, stable=True, return_per_query=True)
    order = torch.argsort(-(x.q @ x.db.t()), dim=1, stable=True)[:, :x.k]
    rel = ranking.label_comparison_fn(x.ql, x.rl)
    return torch.tensor(per_query, dtype=torch.float64), torch.gather(rel, 1, order).sum(1).int()


def same_source(B, D, lwords, kind="grid", seed=11):
    """A minibatch retrieved against itself: (embeddings [B, D], multi-hot labels [B, classes])."""
    classes, p = LABELS[lwords]
    return _EMBED[kind](B, D, seed), multi_hot(B, classes, p, seed + 1)


def _shape_cases():
    """item 1 of the issue: (Q, N, D, lwords, k) on both exact grids -- tile edges of the 256-row staging and of the sort's
    power-of-two padding, one and two label words, k = 1, inside, = N, and the row limit."""
    shapes = [(1, 1, 1, 1, 1), (2, 2, 3, 1, 2)]
    shapes += [(5, n, 16, 1, 10) for n in (63, 64, 65)]
    shapes += [(7, n, 64, 1, k) for n in (255, 256, 257) for k in (1, 100, n)]
    shapes += [(3, 300, 128, 2, 88), (4, 1000, 64, 2, 1000), (2, 2048, 8, 1, 2048)]
    return [Case(*s, kind, 100 + i) for i, s in enumerate(shapes) for kind in ("grid", "ties")]


EXACT_CASES = _shape_cases()                                                                   # item 1: against the oracle
COMPOSED_CASES = [Case(5, 300, D, 1, 77, kind, 200 + D) for D in (1, 3, 16, 64, 129, 512) for kind in ("raw", "grid")]   # item 2
PM1_CASES = [Case(6, 300, nbits, 1, 120, "pm1", 300 + nbits) for nbits in (16, 64, 128)]      # item 3
EQUAL_CASES = [Case(4, 300, 16, 1, 300, "equal", 400), Case(4, 300, 16, 2, 150, "equal", 401)]  # item 4
WORD2_CASES = [Case(5, 300, 32, 2, 300, "word2", 500)]                                         # hits in the second word only
ALL_CASES = EXACT_CASES + COMPOSED_CASES + PM1_CASES + EQUAL_CASES + WORD2_CASES


def case_id(c):
    return f"{c.kind}-Q{c.Q}-N{c.N}-D{c.D}-w{c.lwords}-k{c.k}"


def closed_form_equal(case):
    """All scores equal: position p holds row p.  (AP float64 [Q], hits [Q]) from the label pattern alone, the quotients in
    fp32 like the reference's."""
    x = inputs(case)
    rel = ranking.label_comparison_fn(x.ql, x.rl)[:, :x.k]
    aps, hits = [], []
    for row in rel:
        pos = torch.nonzero(row).flatten()
        n = pos.numel()
        quot = torch.arange(1, n + 1, dtype=torch.float32) / (pos + 1).float()
        aps.append(quot.double().sum().item() / n if n else 0.0)
        hits.append(n)
    return torch.tensor(aps, dtype=torch.float64), torch.tensor(hits, dtype=torch.int32)
