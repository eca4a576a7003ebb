"""The calculator's routes on the GPU, at the smallest shapes at which each can go wrong.  Every metric is one body over a
ranking session (RankCache): the unshared calculator (a session per metric call), a calculator on a shared session and
device='cpu' must agree -- per-query AP bit for bit, unshared and shared dictionaries exactly, host scalars within the
rounding of their last reduction -- and take the route the shape calls for, counted at the attributes of engine/hamming.py."""
import functools

import pytest
import torch

from wvhash import synth
from wvhash.engine import get_accuracy_calculator
from wvhash.engine import hamming as H
from wvhash.engine.accuracy_calculator import RankCache

pytestmark = pytest.mark.gpu

COUNTED = ("hamming_map_at_k", "hamming_map_at_ks", "hamming_topk", "map_at_k", "map_at_ks")
FUSED = {"hamming_map_at_k": 1}
# name: Q, N, bits, classes (0: 1-D ids of 10 classes), k, ks, same source, calls of one calculate_maphashing(k)
CASES = {"fused": (33, 1000, 64, 38, 100, (20, 100, 1000), False, FUSED),
         "two_label_words": (17, 700, 128, 80, 50, (50, 700), False, FUSED),
         "wide_labels": (9, 500, 64, 130, 50, (50,), False, {"hamming_topk": 1, "map_at_k": 1}),      # fused refused
         "class_ids": (9, 400, 32, 0, 40, (40,), False, FUSED),
         "virtual_shards": (8, 32769, 64, 38, 50, (50,), False, FUSED),
         "same_source": (12, 600, 64, 38, 30, (30,), True, FUSED)}
# float64 means of at most 33 exact quotients: the tolerance of tests/test_gpu_ranking.py's host-against-GPU comparison.
# A bit's balance is 1 - 2 |count / N - 0.5| in float32: the GPU divides by the scalar N as a multiplication with 1 / N, one ulp
# (<= 2^-24) off the host's quotient; doubled, plus the final subtraction's rounding on either side (2 * 2^-25): within 2^-22.
# bit_balance is their float32 mean over nbits <= 128 values in [0, 1]: the two summation orders add (nbits - 1) * 2^-24.
TOL = {"worst_bit_balance": 2.0 ** -22, "bit_balance": 2.0 ** -22 + 127 * 2.0 ** -24, "pr_rc": 0.0}


@functools.lru_cache(maxsize=None)
def _pair(name):
    Q, N, bits, classes, _, _, same, _ = CASES[name]
    if classes == 0:
        g = torch.Generator().manual_seed(7)
        ql, rl = torch.randint(0, 10, (Q,), generator=g), torch.randint(0, 10, (N,), generator=g)
        q, r = synth.random_codes(Q, N, bits, seed=9)
        return q, ql, r, rl
    ql, rl = synth.multi_hot_labels(Q, classes, 0.10, 1), synth.multi_hot_labels(N, classes, 0.10, 2)
    q, r = synth.structured_codes(ql, bits, 3, 4), synth.structured_codes(rl, bits, 3, 5)
    return (r[:Q], rl[:Q], r, rl) if same else (q, ql, r, rl)


def _calculator(k, **kw):
    return get_accuracy_calculator(k=k, distance_metric="hamming", with_faiss=False, pr_rc_path=None, **kw)


class _Spy:
    """Counts the calls of engine/hamming.py's attributes: (arguments, answered None) per call."""

    def __init__(self, monkeypatch):
        self.calls = {n: [] for n in COUNTED}
        for n in COUNTED:
            monkeypatch.setattr(H, n, functools.partial(self._call, n, getattr(H, n)))

    def _call(self, name, real, *a, **kw):
        got = real(*a, **kw)
        self.calls[name].append((a, got is None))
        return got

    def take(self):
        """{name: number of calls} of the calls since the last take (names without a call left out), and the calls."""
        calls, self.calls = self.calls, {n: [] for n in COUNTED}
        return {n: len(c) for n, c in calls.items() if c}, calls


@pytest.mark.parametrize("name", list(CASES))
def test_unshared_shared_and_host_agree_and_take_the_route_of_the_shape(name, monkeypatch):
    Q, N, bits, classes, k, ks, same, route = CASES[name]
    q, ql, r, rl = _pair(name)
    dev = [t.cuda() for t in (q, ql, r, rl)]
    spy = _Spy(monkeypatch)

    # one cut-off: the unshared calculator and a shared session with that one cut-off (the single-k entry points)
    value, ap = _calculator(k).calculate_maphashing(*dev, k, ref_includes_query=same, return_per_query=True)
    counts, calls = spy.take()
    assert counts == route, counts
    if name == "two_label_words":
        assert calls["hamming_map_at_k"][0][0][3].shape[1] == 2                  # two packed label words per query
    if name == "virtual_shards":
        db = calls["hamming_map_at_k"][0][0][1]
        assert len(db.parts) == 2 and not calls["hamming_map_at_k"][0][1]        # two parts, answered by the fused route
    one = _calculator(k, rank_cache=RankCache(ks=(k,)))
    value_one, ap_one = one.calculate_maphashing(*dev, k, ref_includes_query=same, return_per_query=True)
    assert spy.take()[0] == route and value_one == value and torch.equal(ap_one, ap)
    value_host, ap_host = _calculator(k, device="cpu").calculate_maphashing(q, ql, r, rl, k, ref_includes_query=same, return_per_query=True)
    assert spy.take()[0] == {} and ap_host.device.type == "cpu"                  # the host backend never touches engine/hamming.py
    assert torch.equal(ap.cpu(), ap_host) and abs(value - value_host) < 1e-9
    if classes == 0:                                                             # class ids are one-hot packed inside the session
        onehot = [(t.unsqueeze(1) == torch.arange(10)).float().cuda() for t in (ql, rl)]
        assert torch.equal(_calculator(k).calculate_maphashing(dev[0], onehot[0], dev[2], onehot[1], k, return_per_query=True)[1], ap)
        spy.take()

    # several cut-offs: one fused multi-k pass, unshared (calculate_maphashing_at) and from a shared session
    many = _calculator(k, rank_cache=RankCache(ks=ks))
    value_many, ap_many = many.calculate_maphashing(*dev, k, ref_includes_query=same, return_per_query=True)
    counts, calls = spy.take()
    if len(ks) > 1:
        assert counts == {"hamming_map_at_ks": 1} and tuple(calls["hamming_map_at_ks"][0][0][5]) == tuple(sorted(ks)), counts
        at = _calculator(k).calculate_maphashing_at(*dev, list(ks), return_per_query=True)
        counts, calls = spy.take()
        assert counts == {"hamming_map_at_ks": 1} and tuple(calls["hamming_map_at_ks"][0][0][5]) == tuple(sorted(ks)), counts
        at_host = _calculator(k, device="cpu").calculate_maphashing_at(q, ql, r, rl, list(ks), return_per_query=True)
        for kk in ks:
            assert torch.equal(at[kk][1].cpu(), at_host[kk][1]) and abs(at[kk][0] - at_host[kk][0]) < 1e-9, kk
        assert at[k][0] == value and torch.equal(at[k][1], ap)
    else:
        assert counts == route, counts
    assert value_many == value and torch.equal(ap_many, ap)

    # the whole dictionary: unshared == shared exactly; the host within the rounding of each metric's last reduction
    spy.take()
    idx, out = _calculator(k).get_accuracy(*dev, same, return_indices=True)
    shared = _calculator(k, rank_cache=RankCache(ks=(k,)))
    idx_shared, out_shared = shared.get_accuracy(*dev, same, return_indices=True)
    counts, calls = spy.take()
    idx_host, out_host = _calculator(k, device="cpu").get_accuracy(q, ql, r, rl, same, return_indices=True)
    assert out == out_shared and set(out) == set(out_host) and {"maphashing", "map", "rpr", "pr", "bit_balance"} <= set(out), (out, out_shared)
    assert torch.equal(idx, idx_shared) and torch.equal(idx.cpu(), idx_host) and tuple(idx.shape) == (Q, k)
    for metric, v in out.items():
        assert abs(v - out_host[metric]) <= TOL.get(metric, 1e-9), (metric, v, out_host[metric])
    if same:                                                                     # the row itself leads its list: trimmed
        assert not bool((idx == torch.arange(Q, device=idx.device)[:, None]).any())
    if name == "virtual_shards":     # a shared session ranks more than 32,768 rows through the prepared database: two parts
        ranked = [c for c in calls["hamming_topk"] if isinstance(c[0][1], H.PreparedDB)]
        assert len(ranked) == 1 and len(ranked[0][0][1].parts) == 2, calls["hamming_topk"]
