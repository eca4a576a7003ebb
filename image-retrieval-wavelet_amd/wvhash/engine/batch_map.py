"""The batch mAP proxy and the fast-eval subset, with the names, signatures and return values of
/root/reference/main/engine/batch_map.py (build_batch_map_calculator :9-20, compute_batch_map :23-36,
build_fast_eval_subset :39-91) and main/engine/make_subset.py (make_subset).

compute_batch_map is the self-retrieval mAP of ONE minibatch -- query set and reference set are both the batch,
k = "max_bin_count" -- on the model's raw train-mode outputs (tanh values or BN logits), logged every step as
``proxy_<metric>`` (base_update.py:70-73, 287-290; engine/train_step.py here).  Under the hamming metric those outputs are
not +-1 codes: the calculator made here has ``soft_codes = True`` and ranks them by inner product like the reference's
calc_hamming_dist does, in one launch (wv_ip_map_at_k).  Any other metric is ``map`` through get_accuracy's k-NN path.
"""
import random
from copy import deepcopy

import torch

from .accuracy_calculator import CustomCalculator


def build_batch_map_calculator(distance_metric, device):
    """-> (calculator, metric name): a light CustomCalculator for the self-retrieval mAP of a single minibatch."""
    metric_name = "maphashing" if distance_metric == "hamming" else "map"
    calculator = CustomCalculator(exclude=["NMI", "AMI"], k="max_bin_count", with_faiss=False,
                                  distance_metric=distance_metric, device=device)
    calculator.soft_codes = True
    return calculator, metric_name


def compute_batch_map(calculator, metric_name, embeddings, labels):
    """-> float: `metric_name` of the batch retrieved against itself.  No graph is kept; [B, 1] labels are class ids."""
    with torch.no_grad():
        embeddings = embeddings.detach()
        if labels.ndim == 2 and labels.size(1) == 1:
            labels = labels.view(-1)
        result = calculator.get_accuracy(query=embeddings, query_labels=labels, reference=embeddings, reference_labels=labels,
                                         embeddings_come_from_same_source=True, include=[metric_name])
    return float(result[metric_name])


def make_subset(dts, idxs, transform=None, mode=None):
    """A deep copy of dataset `dts` reduced to the items `idxs` (in that order), its groupings rebuilt from the kept labels;
    `transform` / `mode` replace the copy's when given."""
    dts = deepcopy(dts)
    dts.paths = [dts.paths[x] for x in idxs]
    dts.labels = [dts.labels[x] for x in idxs]
    if getattr(dts, "super_labels", None) is not None:
        dts.super_labels = [dts.super_labels[x] for x in idxs]
    dts.get_instance_dict()
    dts.get_super_dict()
    if transform is not None:
        dts.transform = transform
    if mode is not None:
        dts.mode = mode
    return dts


def build_fast_eval_subset(dataset, size, min_per_class=2, seed=0):
    """A fixed, stratified self-retrieval subsample of `dataset`, built once so that it can be re-evaluated cheaply and
    consistently across epochs (fast_eval_freq).  Groups come from ``dataset.instance_dict`` ({class or tag index: [item
    indices]}); groups of at least `min_per_class` items are shuffled by `seed` and taken whole, one after the other, until
    `size` items are reached -- an item of several groups is taken once -- then the selection is cut to `size`.
    AttributeError for a dataset without `instance_dict`, ValueError when no group is large enough."""
    rng = random.Random(seed)
    if not hasattr(dataset, "instance_dict"):
        raise AttributeError(f"{type(dataset).__name__} has no `instance_dict`: build_fast_eval_subset groups by "
                             "{class_or_tag_idx: [item indices]} (get_instance_dict() of the hashing datasets)")
    eligible = [members for members in dataset.instance_dict.values() if len(members) >= min_per_class]
    rng.shuffle(eligible)
    selected, seen = [], set()
    for members in eligible:
        if len(selected) >= size:
            break
        for idx in members:
            if idx not in seen:
                seen.add(idx)
                selected.append(idx)
    selected = selected[:size]
    if not selected:
        raise ValueError(f"build_fast_eval_subset: no group of >= {min_per_class} members in "
                         f"{type(dataset).__name__}.instance_dict; disable fast_eval_freq (-1) for this dataset "
                         "instead of evaluating an empty subset")
    subset = make_subset(dataset, selected)
    if hasattr(subset, "_at_R"):
        del subset._at_R
    return subset
