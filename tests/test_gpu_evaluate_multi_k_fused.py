"""evaluate_multi_k and evaluate_sharded with several cut-offs answered from ONE ranking pass.

Without a k-NN metric in the run no [Q, k_max] list exists at all: maphashing of every k comes from the fused ranking + AP
pass (wv_hamming_map_at_ks) -- hamming_topk is not called once.  With a k-NN metric the lists it needs are ranked once and
read once for all k (wv_map_at_ks).  evaluate_sharded takes a sequence of k: same collectives as for one k, sized by the
largest, values equal to its single-k runs."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from PIL import Image
from torch.utils.data import Dataset

from wvhash import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_LIST = (20, 160, 55)
KNN_METRICS = ["precision_at_1", "rpr", "pr", "pr_rc", "mean_reciprocal_rank", "r_precision"]
COLUMNS = ("maphashing_level0", "map_level0", "bit_balance_level0", "worst_bit_balance_level0")


class SynthHashing(Dataset):
    """{"image","label","path"} items like MIRFlickrHashing.__getitem__ (flikr_coco.py:52-63)."""

    def __init__(self, n, seed, transform):
        self.imgs = synth.natural_images(n, 224, 224, seed=seed)
        self.labels = synth.multi_hot_labels(n, 38, 0.10, seed)
        self.transform = transform

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        return {"image": self.transform(Image.fromarray(self.imgs[i])), "label": self.labels[i], "path": str(i)}


def build():
    """A stub-backbone hashing model and {"test": 24 queries, "gallery": 160 rows} (the shape of tests/test_gpu_evaluate.py)."""
    from wvhash.models import SharedDinoHashing
    from wvhash.models.vit import tiny_vit
    from wvhash.transforms import SWTTransform
    torch.manual_seed(0)
    fusion = {"type": "cross_attention_advanced", "output_dim": 384, "num_heads": 8, "num_queries": 4,
              "sub_band_dropout_p": 0, "ortho_weight": 0.1}
    net = SharedDinoHashing({"name": "dinov2_vits14", "frozen": True}, fusion, {"nbits": 64}, backbone=tiny_vit())
    net.hash_fc.weight.data.mul_(50)
    for name, prm in net.named_parameters():
        if name.endswith(".gamma"):
            prm.data.fill_(1.0)
    net = net.cuda().eval().set_wavelet(level=1, wavelet="haar")
    tf = SWTTransform(level=1, wavelet="haar", defer=True)
    return net, {"test": SynthHashing(24, 1, tf), "gallery": SynthHashing(160, 2, tf)}


@pytest.fixture(scope="module")
def setup():
    return build()


def _count_topk(monkeypatch):
    from wvhash.engine import hamming as Hm
    calls, real = [], Hm.hamming_topk
    monkeypatch.setattr(Hm, "hamming_topk", lambda *a, **kw: (calls.append(a[3]), real(*a, **kw))[1])
    return calls, lambda: monkeypatch.setattr(Hm, "hamming_topk", real)


def test_no_knn_metric_no_list_every_k_from_the_fused_pass(setup, monkeypatch):
    from wvhash.engine import evaluate, evaluate_multi_k
    from wvhash.engine import hamming as Hm
    net, dts = setup
    kw = dict(test_dataset=dts, epoch=3, batch_size=32, num_workers=0, distance_metric="hamming", exclude=KNN_METRICS + ["map"])
    calls, restore = _count_topk(monkeypatch)
    fused, real_ks = [], Hm.hamming_map_at_ks
    monkeypatch.setattr(Hm, "hamming_map_at_ks", lambda *a, **k_: (fused.append(tuple(a[5])), real_ks(*a, **k_))[1])
    res = evaluate_multi_k(net, k_list=K_LIST, **kw)
    assert calls == [], calls                                    # no ranked list was ever written
    assert fused == [(20, 55, 160)], fused                       # one pass, all the run's cut-offs
    restore()
    assert list(res) == list(K_LIST)
    for k in K_LIST:
        single = evaluate(net, k=k, **kw)["test"]
        assert set(res[k]["test"]) == set(single)
        for key in ("maphashing_level0", "bit_balance_level0", "worst_bit_balance_level0"):
            assert abs(res[k]["test"][key] - single[key]) < 1e-7, (k, key, res[k]["test"][key], single[key])
    assert res[160]["test"]["maphashing_level0"] > 0.0


def test_with_a_knn_metric_one_ranking_and_one_pass_over_its_lists(setup, monkeypatch):
    from wvhash.engine import evaluate, evaluate_multi_k
    from wvhash.engine import hamming as Hm
    net, dts = setup
    kw = dict(test_dataset=dts, epoch=3, batch_size=32, num_workers=0, distance_metric="hamming", exclude=KNN_METRICS)
    calls, restore = _count_topk(monkeypatch)
    from_lists, real_ks = [], Hm.map_at_ks
    monkeypatch.setattr(Hm, "map_at_ks", lambda *a, **k_: (from_lists.append(tuple(a[3])), real_ks(*a, **k_))[1])
    res = evaluate_multi_k(net, k_list=K_LIST, **kw)
    assert calls == [160], calls                                 # the k-NN behind map_level0: one ranking at the largest k
    assert from_lists == [(20, 55, 160)], from_lists             # ... whose lists answer maphashing of every k in one pass
    restore()
    for k in K_LIST:
        single = evaluate(net, k=k, **kw)["test"]
        for key in ("maphashing_level0", "map_level0", "bit_balance_level0"):
            assert abs(res[k]["test"][key] - single[key]) < 1e-7, (k, key)


def test_calculator_answers_cutoffs_of_its_own_like_its_single_k_form():
    from wvhash.engine import CustomCalculator
    ql, rl = synth.multi_hot_labels(12, 38, 0.10, 1), synth.multi_hot_labels(3000, 38, 0.10, 2)
    q, r = synth.random_codes(12, 3000, 64, seed=9)
    calc = CustomCalculator(k=100, distance_metric="hamming", with_faiss=False)
    ks = [100, 1, 3000, 257, 7000, 100]
    got = calc.calculate_maphashing_at(q, ql, r, rl, ks)
    assert list(got) == [100, 1, 3000, 257, 7000]
    for k in ks:
        assert got[k] == calc.calculate_maphashing(q, ql, r, rl, k), k      # 256 threads per query: the same AP bits


def test_evaluate_sharded_takes_a_sequence_of_k_world_size_one(setup):
    from wvhash.engine import evaluate_sharded
    net, dts = setup
    kw = dict(epoch=2, batch_size=32, num_workers=0, distance_metric="hamming")
    multi = evaluate_sharded(net, dts, k=K_LIST, **kw)
    assert list(multi) == list(K_LIST)
    for k in K_LIST:
        single = evaluate_sharded(net, dts, k=k, **kw)
        assert set(single) == {"test"} and set(multi[k]) == {"test"}
        for key in COLUMNS:
            assert multi[k]["test"][key] == single["test"][key], (k, key)
        assert multi[k]["test"]["epoch"] == "2"
    assert multi[160]["test"]["maphashing_level0"] > 0.0


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "image-retrieval-wavelet_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_gpu_evaluate_multi_k_fused import build
    from wvhash import parallel
    from wvhash.engine import evaluate_sharded
    from wvhash.engine import hamming as H
    net, dts = build()
    kw = dict(epoch=2, batch_size=32, num_workers=0, distance_metric="hamming")
    out = {}
    parallel.TRACE = parallel.ExchangeTrace()
    out["multi"] = evaluate_sharded(net, dts, k=K_LIST, **kw)
    out["multi_calls"] = dict(parallel.TRACE.calls)
    out["multi_bytes"] = dict(parallel.TRACE.bytes)
    for k in K_LIST:
        parallel.TRACE = parallel.ExchangeTrace()
        out[k] = evaluate_sharded(net, dts, k=k, **kw)
        out[(k, "calls")], out[(k, "bytes")] = dict(parallel.TRACE.calls), dict(parallel.TRACE.bytes)
    # the search alone: one all_gather (codes | label words), one all_to_all (histogram | relevance string)
    n_db, nbits, ql_n = 3001, 64, 7
    labels_q, labels_r = synth.multi_hot_labels(world * ql_n, 38, 0.10, 1), synth.multi_hot_labels(n_db, 38, 0.10, 2)
    q, r = synth.random_codes(world * ql_n, n_db, nbits, seed=5)
    lo, hi, _ = parallel.shard_bounds(n_db, world, rank)
    qp = H.pack_codes(q[rank * ql_n:(rank + 1) * ql_n].cuda())
    qlp = H.pack_labels(labels_q[rank * ql_n:(rank + 1) * ql_n].cuda())
    rlp = H.pack_labels(labels_r.cuda())
    shard, shard_labels = H.PreparedDB(H.pack_codes(r[lo:hi].cuda()), nbits), H.PreparedLabels(rlp[lo:hi].contiguous())
    ks = (700, 20, 1501, 256)
    parallel.TRACE = parallel.ExchangeTrace()
    ap, nrel, need = parallel.sharded_hamming_map_at_k(qp, qlp, shard, shard_labels, nbits, ks, n_db, None)
    out["search_calls"] = dict(parallel.TRACE.calls)
    parallel.TRACE = None
    same = tuple(ap.shape) == (ql_n, len(ks))
    full_idx, _ = H.hamming_topk(qp, H.pack_codes(r.cuda()), nbits, max(ks), want_dist=False)
    for i, k in enumerate(ks):
        ap1, nrel1, _ = parallel.sharded_hamming_map_at_k(qp, qlp, shard, shard_labels, nbits, k, n_db, None)
        ap2, nrel2 = H.map_at_k(full_idx, qlp, rlp, k=k)
        same = same and torch.equal(ap[:, i], ap1) and torch.equal(nrel[:, i], nrel1)
        same = same and torch.equal(ap[:, i], ap2) and torch.equal(nrel[:, i], nrel2) and bool((nrel2 > 0).all() or k < 64)
    out["search_equal"] = same
    torch.save(out, os.path.join(out_dir, f"m{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_sharded_takes_a_sequence_of_k_two_ranks(tmp_path):
    """Two gloo ranks on one GPU (as tests/test_gpu_parallel.py): every k of the sequence gets the numbers of its own
    single-k run; the multi-k run issues the collectives of ONE single-k run -- in the search one all_gather and one
    all_to_all --, the exchange sized by the largest k."""
    port = 29300 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        got = torch.load(os.path.join(tmp_path, f"m{rank}.pt"))
        assert list(got["multi"]) == list(K_LIST)
        for k in K_LIST:
            for key in COLUMNS:
                assert got["multi"][k]["test"][key] == got[k]["test"][key], (rank, k, key)
        assert got["multi_calls"] == got[(160, "calls")], (got["multi_calls"], got[(160, "calls")])
        assert got["multi_calls"]["all_to_all"] == 1
        # the wire is the largest k's; the only extra bytes are the AP sums of the other cut-offs in the final all-reduce
        assert got["multi_bytes"]["all_to_all"] == got[(160, "bytes")]["all_to_all"]
        assert got["multi_bytes"]["all_gather"] == got[(160, "bytes")]["all_gather"]
        assert got["multi_bytes"]["all_reduce"] == got[(160, "bytes")]["all_reduce"] + 8 * (len(K_LIST) - 1)
        assert got["search_calls"]["all_gather"] == 1 and got["search_calls"]["all_to_all"] == 1, got["search_calls"]
        assert got["search_equal"]
        assert got["multi"][160]["test"]["maphashing_level0"] > 0.0
