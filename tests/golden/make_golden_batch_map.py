#!/usr/bin/env python3
"""Regenerates tests/golden/batch_map_golden.json:   python tests/golden/make_golden_batch_map.py <root of the reference checkout>

The file pins build_fast_eval_subset / make_subset against the REFERENCE's own code.  build_fast_eval_subset
(main/engine/batch_map.py) and make_subset (main/engine/make_subset.py) need only `random` and `deepcopy`; their FunctionDef
nodes are cut out of the reference files with `ast` at generation time (the `_cut` pattern of make_golden.py -- nothing of
the source is stored), compiled unmodified and run on a seeded synthetic dataset.  Stored: the dataset's label rows, and per
(size, min_per_class, seed) the index list the reference selected and the subset's regrouped instance_dict; the exception
type of its two error conditions.  Data only.  No test reads the reference; tests read the .json.
"""
import ast
import json
import os
import random
import sys
from collections import defaultdict
from copy import deepcopy

HERE = os.path.dirname(os.path.abspath(__file__))
N_ITEMS, N_CLASSES, P_TAG = 600, 12, 0.2
SIZES, MIN_PER_CLASS, SEEDS = (10, 500), (2, 3), (0, 5)


def _cut(path, names):
    with open(path, "r") as f:
        tree = ast.parse(f.read(), filename=path)
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    missing = [n for n in names if n not in found]
    if missing:
        raise RuntimeError(f"{path}: {missing} not found")
    return [found[n] for n in names]


def load_reference(ref_root):
    funcs = _cut(os.path.join(ref_root, "main", "engine", "make_subset.py"), ["make_subset"]) + \
        _cut(os.path.join(ref_root, "main", "engine", "batch_map.py"), ["build_fast_eval_subset"])
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"random": random, "deepcopy": deepcopy}
    exec(compile(mod, "<reference batch_map.py / make_subset.py (cut)>", "exec"), ns)
    return ns["build_fast_eval_subset"]


def label_rows():
    """0/1 rows: Bernoulli tags, a class with exactly two members (eligible at min_per_class 2 only), rows without a tag"""
    rng = random.Random(1234)
    rows = [[int(rng.random() < P_TAG) for _ in range(N_CLASSES - 1)] + [0] for _ in range(N_ITEMS)]
    rows[17][N_CLASSES - 1] = rows[401][N_CLASSES - 1] = 1
    assert any(sum(r) == 0 for r in rows)
    return rows


class Synthetic(object):
    """What the two functions touch of a hashing dataset: paths (here: the item's own index), labels, the groupings"""

    def __init__(self, rows):
        self.paths = list(range(len(rows)))
        self.labels = [list(r) for r in rows]
        self.transform, self.mode = None, "train"
        self.get_instance_dict()

    def get_instance_dict(self):
        self.instance_dict = defaultdict(list)
        for i, row in enumerate(self.labels):
            for c, v in enumerate(row):
                if v == 1:
                    self.instance_dict[c].append(i)

    def get_super_dict(self):
        pass


class NoGroups(object):
    paths, labels = [0, 1], [[1], [1]]


def main(ref_root):
    build = load_reference(ref_root)
    rows = label_rows()
    out = {"labels": rows, "cases": [], "errors": {}}
    for size in SIZES:
        for mpc in MIN_PER_CLASS:
            for seed in SEEDS:
                sub = build(Synthetic(rows), size, min_per_class=mpc, seed=seed)
                assert len(sub.paths) == min(size, len(sub.paths)) and len(set(sub.paths)) == len(sub.paths)
                out["cases"].append({"size": size, "min_per_class": mpc, "seed": seed, "selected": list(sub.paths),
                                     "instance_dict": [[k, list(v)] for k, v in sub.instance_dict.items()]})
                print(size, mpc, seed, len(sub.paths), sub.paths[:8])
    sel = {(c["min_per_class"], c["seed"]): c["selected"] for c in out["cases"] if c["size"] == 500}
    assert sel[(2, 0)] != sel[(3, 0)] and sel[(2, 0)] != sel[(2, 5)]          # both knobs change the selection
    for name, dataset, kwargs in (("no_instance_dict", NoGroups(), {}), ("no_eligible_group", Synthetic(rows[:40]), {"min_per_class": 10 ** 6})):
        try:
            build(dataset, 10, **kwargs)
            raise AssertionError(name)
        except (AttributeError, ValueError) as e:
            out["errors"][name] = type(e).__name__
    path = os.path.join(HERE, "batch_map_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes", out["errors"])
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
