"""wvhash.engine.batch_map without a GPU: the fast-eval subset against index lists the reference's own function selected
(tests/golden/batch_map_golden.json, made by tests/golden/make_golden_batch_map.py), compute_batch_map's return value and
label handling, and the proxy hook of train_step / backward_step."""
import json
import os

import pytest
import torch

import ip_map_cases as C
from oracle import ranking
from wvhash import datasets, engine
from wvhash.engine import batch_map


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "batch_map_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def split_dataset(golden, tmp_path_factory):
    """The golden label rows as a split-file dataset: item i is file i.jpg"""
    root = tmp_path_factory.mktemp("split")
    with open(root / "train.txt", "w") as f:
        for i, row in enumerate(golden["labels"]):
            f.write(f"{i}.jpg " + " ".join(str(v) for v in row) + "\n")
    return datasets.COCOHashing(str(root), mode="train")


def _items(ds):
    return [int(os.path.basename(p)[:-4]) for p in ds.paths]


def test_the_four_names_are_exported():
    for name in ("build_batch_map_calculator", "compute_batch_map", "build_fast_eval_subset", "make_subset"):
        assert getattr(engine, name) is getattr(batch_map, name) and name in engine.__all__


def test_get_instance_dict_rebuilds_what_init_built(split_dataset, golden):
    built = {k: list(v) for k, v in split_dataset.instance_dict.items()}
    want = {}
    for i, row in enumerate(golden["labels"]):
        for c, v in enumerate(row):
            if v:
                want.setdefault(c, []).append(i)
    assert built == want and list(built) == list(want)                     # same groups, same order of the groups
    split_dataset.get_instance_dict()
    assert {k: list(v) for k, v in split_dataset.instance_dict.items()} == built
    assert split_dataset.get_super_dict() is None


def test_fast_eval_subset_selects_what_the_reference_selects(split_dataset, golden):
    assert {(c["size"], c["min_per_class"], c["seed"]) for c in golden["cases"]} == \
        {(s, m, d) for s in (10, 500) for m in (2, 3) for d in (0, 5)}
    before = list(split_dataset.paths)
    for c in golden["cases"]:
        sub = batch_map.build_fast_eval_subset(split_dataset, c["size"], min_per_class=c["min_per_class"], seed=c["seed"])
        assert _items(sub) == c["selected"], c["size"]
        assert [[k, list(v)] for k, v in sub.instance_dict.items()] == c["instance_dict"]
        assert len(sub) == len(c["selected"]) and len(sub.labels) == len(sub)
        for j in (0, len(sub) - 1):
            assert torch.equal(sub.labels[j], split_dataset.labels[c["selected"][j]])
    assert split_dataset.paths == before                                    # the subset is a copy


def test_make_subset_sets_transform_mode_and_super_labels(split_dataset):
    marker = object()
    sub = batch_map.make_subset(split_dataset, [5, 3, 3], transform=marker, mode="query")
    assert _items(sub) == [5, 3, 3] and sub.transform is marker and sub.mode == "query"
    assert split_dataset.transform is None and split_dataset.mode == "train"
    split_dataset.super_labels = list(range(len(split_dataset)))
    try:
        assert batch_map.make_subset(split_dataset, [7, 2]).super_labels == [7, 2]
    finally:
        del split_dataset.super_labels


def test_fast_eval_subset_error_conditions(split_dataset, golden):
    class NoGroups(object):
        paths, labels = [0, 1], [[1], [1]]
    errors = {"AttributeError": AttributeError, "ValueError": ValueError}
    with pytest.raises(errors[golden["errors"]["no_instance_dict"]], match="instance_dict"):
        batch_map.build_fast_eval_subset(NoGroups(), 10)
    with pytest.raises(errors[golden["errors"]["no_eligible_group"]], match="fast_eval_freq"):
        batch_map.build_fast_eval_subset(split_dataset, 10, min_per_class=10 ** 6)
    assert golden["errors"] == {"no_instance_dict": "AttributeError", "no_eligible_group": "ValueError"}


def test_subset_drops_a_cached_at_R(split_dataset):
    split_dataset._at_R = 7
    try:
        assert not hasattr(batch_map.build_fast_eval_subset(split_dataset, 10), "_at_R")
    finally:
        del split_dataset._at_R


# ------------------------------------------------------------------------------------------------- compute_batch_map
def test_build_batch_map_calculator_follows_the_reference():
    calc, name = batch_map.build_batch_map_calculator("hamming", "cpu")
    assert name == "maphashing" and calc.soft_codes is True and calc.k == "max_bin_count" and calc.with_faiss is False
    assert calc.distance_metric == "hamming" and calc.host
    calc, name = batch_map.build_batch_map_calculator("cosine", "cpu")
    assert name == "map" and calc.distance_metric == "cosine"


def test_compute_batch_map_returns_a_float_equal_to_the_oracle():
    calc, name = batch_map.build_batch_map_calculator("hamming", "cpu")
    emb, lab = C.same_source(96, 64, 1)
    emb.requires_grad_()
    got = batch_map.compute_batch_map(calc, name, emb, lab)
    assert type(got) is float
    ref = ranking.calculate_maphashing(emb.detach(), lab, emb.detach(), lab, "max_bin_count", ref_includes_query=True, stable=True)
    assert ref > 0 and abs(got - ref) <= C.AP_TOL


def test_compute_batch_map_flattens_column_labels():
    calc, name = batch_map.build_batch_map_calculator("hamming", "cpu")
    emb, _ = C.same_source(64, 32, 1)
    ids = torch.randint(0, 7, (64, 1), generator=torch.Generator().manual_seed(3))
    got = batch_map.compute_batch_map(calc, name, emb, ids)
    assert type(got) is float and got == batch_map.compute_batch_map(calc, name, emb, ids.view(-1))
    onehot = (ids == torch.arange(7)).float()
    assert abs(got - ranking.calculate_maphashing(emb, onehot, emb, onehot, "max_bin_count", ref_includes_query=True,
                                                  stable=True)) <= C.AP_TOL


def test_compute_batch_map_other_metrics_are_map_through_the_knn_path():
    calc, name = batch_map.build_batch_map_calculator("cosine", "cpu")
    emb, lab = C.same_source(64, 32, 1, kind="raw")
    emb = torch.nn.functional.normalize(emb, dim=1)
    got = batch_map.compute_batch_map(calc, name, emb, lab)
    assert type(got) is float and 0.0 < got <= 1.0


# ------------------------------------------------------------------------------------------------- train_step
class _PairLoss(torch.nn.Module):
    def forward(self, scores, same):
        return (scores / scores.shape[0] - same) ** 2


def _step_world(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 4 * 4, 16), torch.nn.Tanh())
    images = torch.randn(24, 3, 4, 4)
    labels = C.multi_hot(24, 38, 0.10, 5)
    return net, images, labels, [(_PairLoss(), 1.0)], [torch.optim.SGD(net.parameters(), lr=0.1)]


@pytest.mark.parametrize("sub_batch", [None, 10])
def test_train_step_logs_exactly_the_proxy_key(sub_batch):
    calc, name = batch_map.build_batch_map_calculator("hamming", "cpu")
    net, images, labels, criteria, opts = _step_world()
    with torch.no_grad():
        emb = net(images)                                       # the step's embeddings: the parameters before the update
    want = batch_map.compute_batch_map(calc, name, emb, labels)
    plain = engine.train_step(*_step_world(), autocast_dtype=None, sub_batch=sub_batch)       # the same world, no proxy
    logs = engine.train_step(net, images, labels, criteria, opts, autocast_dtype=None, sub_batch=sub_batch,
                             batch_map_calculator=calc, batch_map_metric=name)
    assert set(logs) == set(plain) | {"proxy_maphashing"} and "proxy_maphashing" not in plain
    assert type(logs["proxy_maphashing"]) is float and logs["proxy_maphashing"] == want and want > 0.0
    assert {k: v for k, v in logs.items() if k != "proxy_maphashing"} == plain       # the step itself is unchanged


def test_backward_step_takes_the_same_arguments():
    calc, name = batch_map.build_batch_map_calculator("cosine", "cpu")
    net, images, labels, criteria, _ = _step_world()
    logs = engine.backward_step(net, images, labels, criteria, autocast_dtype=None, batch_map_calculator=calc, batch_map_metric=name)
    assert "proxy_map" in logs and 0.0 <= logs["proxy_map"] <= 1.0
