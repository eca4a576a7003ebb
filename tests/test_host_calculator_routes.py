"""The calculator's routes on the host backend (device='cpu'; no GPU is touched): every metric is one body over a ranking
session (RankCache).  A session shared by three calculators returns exactly what three unshared calculators return and
ranks once; an unshared calculator asks the single-k entry point; get_knn(device='cpu') is hamming_topk / knn_float_host
called directly; a session and a calculator of different backends refuse each other."""
import pytest
import torch

from wvhash import _lib, synth
from wvhash.engine import CustomCalculator, get_accuracy_calculator, get_knn
from wvhash.engine import hamming_host as HH
from wvhash.engine.accuracy_calculator import RankCache
from wvhash.engine.get_knn import knn_float_host

Q, N, NBITS, CLASSES = 24, 160, 64, 38
KS = (20, 160, 55)
OPT_IN = ["precision_hamming_radius", "pr_curve_hamming", "ndcg_hamming"]


@pytest.fixture(scope="module")
def pair():
    ql, rl = synth.multi_hot_labels(Q, CLASSES, 0.10, 1), synth.multi_hot_labels(N, CLASSES, 0.10, 2)
    return synth.structured_codes(ql, NBITS, 3, 4), ql, synth.structured_codes(rl, NBITS, 3, 5), rl


def _calculator(k, **kw):
    return get_accuracy_calculator(k=k, device="cpu", distance_metric="hamming", with_faiss=False, pr_rc_path=None, **kw)


def _count(monkeypatch, *names):
    """Calls of hamming_host.<name>, by their fourth positional argument (hamming_topk: k; map_at_k(s): the cut-offs)."""
    calls = {n: [] for n in names}
    for n in names:
        real = getattr(HH, n)
        monkeypatch.setattr(HH, n, lambda *a, _n=n, _real=real, **kw: (calls[_n].append(a[3] if len(a) > 3 else kw.get("k")),
                                                                      _real(*a, **kw))[1])
    return calls


def _run(calc, pair):
    q, ql, r, rl = pair
    out = calc.get_accuracy(q, ql, r, rl, False, include=calc.get_curr_metrics() + OPT_IN)
    assert set(OPT_IN) < set(out) and {"maphashing", "map", "rpr", "pr", "pr_rc", "bit_balance"} <= set(out)
    curves = [t.clone() for t in calc.last_pr_rc + calc.last_pr_curve_hamming]
    per_query = calc.calculate_maphashing(q, ql, r, rl, calc.k, return_per_query=True)[1]
    return out, curves, per_query


def test_shared_host_session_equals_unshared_and_ranks_once(pair, monkeypatch):
    calls = _count(monkeypatch, "hamming_topk", "map_at_k", "map_at_ks")
    cache = RankCache(ks=KS, device="cpu")
    shared = [_run(_calculator(k, rank_cache=cache), pair) for k in KS]
    assert calls["hamming_topk"] == [160], calls                       # one ranking, at the largest cut-off
    assert [tuple(c) for c in calls["map_at_ks"]] == [(20, 55, 160)], calls       # ... whose lists answer maphashing of every k
    for k, (out, curves, per_query) in zip(KS, shared):
        for n in calls:
            calls[n].clear()
        want, want_curves, want_per_query = _run(_calculator(k), pair)
        assert calls["map_at_ks"] == [] and k in calls["map_at_k"], calls         # one cut-off: the single-k entry point
        assert out == want, (k, out, want)
        assert all(torch.equal(a, b) for a, b in zip(curves, want_curves))
        assert torch.equal(per_query, want_per_query)
    assert shared[1][0]["maphashing"] > 0.0


@pytest.mark.parametrize("same_source", [False, True])
def test_get_knn_on_the_host_is_the_primitives_called_directly(pair, same_source):
    q, _, r, _ = pair
    if same_source:
        q = r[:12]
    first, k = int(same_source), 30
    idx, ip = get_knn(r, q, k, same_source, with_faiss=False, distance_metric="hamming", device="cpu")
    want_idx, want_d = HH.hamming_topk(HH.pack_codes(q), HH.pack_codes(r), NBITS, k + first)
    assert idx.dtype == torch.int64 and torch.equal(idx, want_idx[:, first:].long())
    assert torch.equal(ip, (float(NBITS) - 2.0 * want_d.float())[:, first:])
    g = torch.Generator().manual_seed(5)
    rf = torch.randn(N, 32, generator=g)
    qf = rf[:12] if same_source else torch.randn(Q, 32, generator=g)
    for metric, faiss, c_metric in (("cosine", True, _lib.WV_METRIC_IP), ("l2", True, _lib.WV_METRIC_L2_SQUARED),
                                    ("l2", False, _lib.WV_METRIC_L2)):
        idx, val = get_knn(rf, qf, k, same_source, with_faiss=faiss, distance_metric=metric, device=torch.device("cpu"))
        want_val, want_idx = knn_float_host(rf, qf, k + first, c_metric)
        assert torch.equal(idx, want_idx[:, first:].long()) and torch.equal(val, want_val[:, first:]), (metric, faiss)
    if same_source:
        assert not (idx == torch.arange(12)[:, None]).any()            # column 0 (the row itself) stripped
    with pytest.raises(RuntimeError, match="k out of range"):
        get_knn(r, q, N + 1 - first, same_source, distance_metric="hamming", device="cpu")


def test_session_and_calculator_of_different_backends_refuse_each_other():
    with pytest.raises(ValueError, match="a shared RankCache holds GPU lists"):
        CustomCalculator(k=5, device="cpu", distance_metric="hamming", rank_cache=RankCache())
    with pytest.raises(ValueError, match="a shared RankCache holds host lists"):
        CustomCalculator(k=5, distance_metric="hamming", rank_cache=RankCache(device="cpu"))
    assert CustomCalculator(k=5, device=torch.device("cpu"), rank_cache=RankCache(device="cpu")).host
