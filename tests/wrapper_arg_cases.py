"""Shared by tests/test_wrapper_args.py and tests/test_gpu_wrapper_args.py: the table of the public wrappers of
wvhash/engine/hamming.py (one row each: its tensor arguments with their declared dtype and kind, canonical arguments, the
call, the expected outputs), the tensor forms a caller may hand over (accepted: the wrapper must compute what it computes
for the canonical tensor; refused: ValueError before any entry point runs), and the worlds the rows are run in.  Everything
expected is plain torch on the host (oracle/ranking.py and a few lines here): no kernel, no library call."""
import functools

import torch

from oracle import ranking
from wvhash import synth
from wvhash.engine import hamming as H

ROWS, PITCH, WRITTEN, INDEX = "rows", "pitch", "written", "index"      # the gate's kinds (wvhash/engine/_args.py)
Q = 37
KS = [1, 64, 100]
WORLDS = [(3000, 64, 38), (3000, 128, 80), (257, 64, 80), (257, 128, 38)]     # (N, nbits, classes): both N, every width pair
SHARD_ROWS, SHARD_K = 1500, 100                                              # two shards of the 3000-row worlds
WORKSPACE_BYTES = 4 << 20        # a caller's TopkWorkspace in the table: larger than any of these shapes needs (asserted on the GPU)
EXACT, AP, DCG, SHAPE = "exact", "ap", "dcg", "shape"                        # how an output is held against its expectation


def pack_bits(x):
    """bool [rows, n] -> int64 [rows, ceil(n / 64)], bit j of word w = x[:, 64 w + j]: what pack_codes / pack_labels make"""
    rows, n = x.shape
    words = (n + 63) // 64
    b = torch.zeros((rows, words * 64), dtype=torch.int64)
    b[:, :n] = x.long()
    return (b.view(rows, words, 64) << torch.arange(64, dtype=torch.int64)).sum(2)


def cum_hist(D, nbits):
    """int32 [Q, nbits + 2]: cum[q, b] = rows with distance < b"""
    return torch.stack([(D < b).sum(1) for b in range(nbits + 2)], dim=1).int()


class World:
    """One database and query set on the host with everything the rows need, made once: structured codes plus a block of
    duplicated rows (their labels differ), so that equal distances straddle the k-th place and the two shards."""

    def __init__(self, N, nbits, classes):
        self.N, self.nbits, self.classes, self.Q = N, nbits, classes, Q
        self.ql, self.rl = synth.multi_hot_labels(Q, classes, 0.1, 1), synth.multi_hot_labels(N, classes, 0.1, 2)
        self.q, self.r = synth.structured_codes(self.ql, nbits, 3, 4), synth.structured_codes(self.rl, nbits, 3, 5)
        dup = min(64, N // 4)
        self.r[N // 2:N // 2 + dup] = self.r[:dup]
        self.ks = [100] if N > 257 else [100, N]
        self.qp, self.rp = pack_bits(self.q > 0), pack_bits(self.r > 0)
        self.qlp, self.rlp = pack_bits(self.ql > 0), pack_bits(self.rl > 0)
        self.D = ranking.hamming_matrix_u8(self.q, self.r)
        self.rel = ranking.label_comparison_fn(self.ql, self.rl)
        self.overlap = self.ql.long() @ self.rl.long().t()
        order, d = ranking.hamming_topk_stable(self.q, self.r, N)
        self.order, self.order_d = order.int(), d.to(torch.uint8)
        self.cum = cum_hist(self.D, nbits)
        self.cumrel = cum_hist(torch.where(self.rel, self.D, torch.full_like(self.D, nbits + 9)), nbits)
        self.hist = torch.stack([torch.bincount(row, minlength=64 * self.qlp.shape[1] + 1) for row in self.overlap]).int()
        self.shards = N == 2 * SHARD_ROWS
        if self.shards:
            k = SHARD_K
            parts = [ranking.hamming_topk_stable(self.q, self.r[lo:lo + SHARD_ROWS], k) for lo in (0, SHARD_ROWS)]
            self.rows16 = torch.stack([p[0].to(torch.int16) for p in parts])
            self.gidx = torch.stack([(p[0] + lo).int() for p, lo in zip(parts, (0, SHARD_ROWS))])
            self.gdist = torch.stack([p[1].to(torch.uint8) for p in parts])
            self.cums = torch.stack([cum_hist(self.D[:, lo:lo + SHARD_ROWS], nbits) for lo in (0, SHARD_ROWS)])
            T = (self.cums.sum(0)[:, 1:] >= k).int().argmax(dim=1)                 # every query's global k-th distance
            self.need = torch.gather(self.cums, 2, (T + 1).view(1, Q, 1).expand(2, Q, 1).long()).max().reshape(1).int()
            ld, hw = H.relbits_wire_words(k, nbits), H._hist_words(nbits)
            self.wires = torch.zeros((2, Q, ld), dtype=torch.int64)
            for g, (p, lo) in enumerate(zip(parts, (0, SHARD_ROWS))):
                self.wires[g].view(torch.int32)[:, :nbits + 2] = self.cums[g]
                self.wires[g, :, hw:] = pack_bits(torch.gather(self.rel[:, lo:lo + SHARD_ROWS], 1, p[0]))

    @functools.lru_cache(maxsize=None)
    def ap(self, k):
        """(ap float64 [Q] of oracle/ranking.py on the canonical order, nrel int32 [Q])"""
        per_query = ranking.calculate_maphashing(self.q, self.ql, self.r, self.rl, k, stable=True, return_per_query=True)[1]
        return torch.tensor(per_query, dtype=torch.float64), self.hits(k)[:, -1].contiguous()

    def aps(self, ks):
        got = [self.ap(k) for k in ks]
        return torch.stack([g[0] for g in got], 1), torch.stack([g[1] for g in got], 1)

    def hits(self, k):
        return torch.gather(self.rel, 1, self.order[:, :k].long()).int().cumsum(1).int()

    def dcg(self, ks):
        """(dcg, idcg) float64 [Q, len(ks)]: gains 2^overlap - 1 over log2(position + 2), the ideal list sorted descending"""
        gains = torch.ldexp(torch.ones((), dtype=torch.float64), self.overlap.int()) - 1.0
        disc = torch.log2(torch.arange(self.N, dtype=torch.float64) + 2.0)
        along = (torch.gather(gains, 1, self.order.long()) / disc).cumsum(1)
        ideal = (gains.sort(1, descending=True)[0] / disc).cumsum(1)
        cols = torch.tensor([k - 1 for k in ks])
        return along[:, cols], ideal[:, cols]


@functools.lru_cache(maxsize=None)
def world(N, nbits, classes):
    return World(N, nbits, classes)


# ------------------------------------------------------------------------------------------------------------- the table
class Arg:
    def __init__(self, name, dtype, kind=ROWS, tied=None):
        """tied: the dimension that must agree with the number of queries / lists (a wrong row count is a refused form)"""
        self.name, self.dtype, self.kind, self.tied = name, dtype, kind, tied

    @property
    def declared(self):
        return torch.int32 if self.dtype == INDEX else self.dtype


class Case:
    def __init__(self, name, args, canon, call, want, twin=False, shards=False, prepare=None):
        """canon(w, k) -> {argument name: canonical host tensor} (names with '_' in front: helpers that are not varied);
        prepare(Hm, a) -> extras made outside the watched call (PreparedDB, PreparedLabels); call(Hm, w, k, a, x) -> tuple of
        output tensors (None where there is none); want(w, k) -> tuple of (expected host tensor, EXACT / AP / DCG / SHAPE);
        twin: hamming_host.py has the wrapper; shards: needs the two-shard worlds."""
        self.name, self.args, self.canon, self.call, self.want = name, args, canon, call, want
        self.twin, self.shards, self.prepare = twin, shards, prepare or (lambda Hm, a: {})

    def __repr__(self):
        return self.name


I64, I32, I16, U8 = torch.int64, torch.int32, torch.int16, torch.uint8
_codes = lambda w, k: {"q_packed": w.qp, "db": w.rp}                                            # noqa: E731
_lists = lambda w, k: {"idx": w.order[:, :k].contiguous(), "qlab_packed": w.qlp, "dblab_packed": w.rlp}   # noqa: E731
_LIST_ARGS = lambda kind: [Arg("idx", INDEX, kind), Arg("qlab_packed", I64, tied=0), Arg("dblab_packed", I64)]   # noqa: E731
_fused = lambda w, k: {"q_packed": w.qp, "qlab_packed": w.qlp, "_rp": w.rp, "_rlp": w.rlp}      # noqa: E731
_FUSED_ARGS = [Arg("q_packed", I64), Arg("qlab_packed", I64, tied=0)]
_prepared = lambda Hm, a: {"db": Hm.PreparedDB(a["_rp"]), "labels": Hm.PreparedLabels(a["_rlp"])}     # noqa: E731
_shard0 = lambda Hm, a: {"db": Hm.PreparedDB(a["_rp"][:SHARD_ROWS]), "labels": Hm.PreparedLabels(a["_rlp"][:SHARD_ROWS])}   # noqa: E731
_topk = lambda w, k: ((w.order[:, :k], EXACT), (w.order_d[:, :k], EXACT))                       # noqa: E731
_need = lambda a: a["need_out"].clone()                                                         # noqa: E731


def _with_workspace(Hm, a):
    ws = Hm.TopkWorkspace()
    ws.buf = a["workspace"]
    return ws


def _prepared_db_call(Hm, w, k, a, x):
    db = Hm.PreparedDB(a["db_packed"], w.nbits)
    return (db.packed,) + tuple(Hm.hamming_topk(a["_qp"], db, w.nbits, k))


def _prepared_labels_call(Hm, w, k, a, x):
    labels = Hm.PreparedLabels(a["dblab_packed"])
    return (labels.packed,) + tuple(Hm.hamming_radius_hist(a["_qp"], x["db"], labels, a["_qlp"], w.nbits))


CASES = [
    Case("bit_counts", [Arg("packed", I64)], lambda w, k: {"packed": w.rp},
         lambda Hm, w, k, a, x: (Hm.bit_counts(a["packed"], w.nbits),),
         lambda w, k: (((w.r > 0).sum(0).int(), EXACT),), twin=True),
    Case("hamming_dist", [Arg("q_packed", I64), Arg("db", I64)], _codes,
         lambda Hm, w, k, a, x: (Hm.hamming_dist(a["q_packed"], a["db"], w.nbits),),
         lambda w, k: ((w.D.to(U8), EXACT),), twin=True),
    Case("hamming_topk", [Arg("q_packed", I64), Arg("db", I64)], _codes,
         lambda Hm, w, k, a, x: Hm.hamming_topk(a["q_packed"], a["db"], w.nbits, k, want_dist=True), _topk, twin=True),
    Case("hamming_topk_want_cum", [Arg("q_packed", I64), Arg("db", I64), Arg("workspace", U8, WRITTEN)],
         lambda w, k: dict(_codes(w, k), workspace=torch.zeros(WORKSPACE_BYTES, dtype=U8)),
         lambda Hm, w, k, a, x: Hm.hamming_topk(a["q_packed"], a["db"], w.nbits, k, workspace=_with_workspace(Hm, a), want_dist=False,
                                                want_cum=True),
         lambda w, k: ((w.order[:, :k], EXACT), None, (w.cum, EXACT))),
    Case("hamming_hist", [Arg("q_packed", I64), Arg("db", I64), Arg("workspace", U8, WRITTEN)],
         lambda w, k: dict(_codes(w, k), workspace=torch.zeros(WORKSPACE_BYTES, dtype=U8)),
         lambda Hm, w, k, a, x: (Hm.hamming_hist(a["q_packed"], a["db"], w.nbits, workspace=_with_workspace(Hm, a)),),
         lambda w, k: ((w.cum, EXACT),)),
    Case("hamming_topk_rows16", [Arg("q_packed", I64), Arg("db", I64)], _codes,
         lambda Hm, w, k, a, x: (Hm.hamming_topk_rows16(a["q_packed"], a["db"], w.nbits, k),),
         lambda w, k: ((w.order[:, :k].to(I16), EXACT),)),
    Case("hamming_shard_prefix", [Arg("q_packed", I64), Arg("db", I64)], _codes,
         lambda Hm, w, k, a, x: Hm.hamming_shard_prefix(a["q_packed"], a["db"], w.nbits, k),
         lambda w, k: ((w.order[:, :k].to(I16), EXACT), (w.cum, EXACT))),
    Case("topk_merge", [Arg("idx_in", INDEX), Arg("dist_in", U8, tied=1)], lambda w, k: {"idx_in": w.gidx, "dist_in": w.gdist},
         lambda Hm, w, k, a, x: Hm.topk_merge(a["idx_in"], a["dist_in"], SHARD_K, w.nbits),
         lambda w, k: _topk(w, SHARD_K), shards=True),
    Case("topk_merge_cum", [Arg("idx_local", I16), Arg("cum", I32, tied=1), Arg("need_out", I32, WRITTEN)],
         lambda w, k: {"idx_local": w.rows16, "cum": w.cums, "need_out": torch.zeros(1, dtype=I32)},
         lambda Hm, w, k, a, x: Hm.topk_merge_cum(a["idx_local"], a["cum"], SHARD_ROWS, SHARD_K, w.nbits, need_out=a["need_out"]) + (_need(a),),
         lambda w, k: _topk(w, SHARD_K) + ((w.need, EXACT),), shards=True),
    Case("rank_from_dist", [Arg("dist_matrix", U8, PITCH)], lambda w, k: {"dist_matrix": w.D.to(U8)},
         lambda Hm, w, k, a, x: Hm.rank_from_dist(a["dist_matrix"], w.nbits, k), _topk),
    Case("map_at_k", _LIST_ARGS(PITCH), _lists, lambda Hm, w, k, a, x: Hm.map_at_k(a["idx"], a["qlab_packed"], a["dblab_packed"], k=k),
         lambda w, k: ((w.ap(k)[0], AP), (w.ap(k)[1], EXACT)), twin=True),
    Case("map_at_ks", _LIST_ARGS(PITCH), _lists, lambda Hm, w, k, a, x: Hm.map_at_ks(a["idx"], a["qlab_packed"], a["dblab_packed"], KS),
         lambda w, k: ((w.aps(KS)[0], AP), (w.aps(KS)[1], EXACT)), twin=True),
    Case("hit_prefix", _LIST_ARGS(ROWS), _lists, lambda Hm, w, k, a, x: (Hm.hit_prefix(a["idx"], a["qlab_packed"], a["dblab_packed"]),),
         lambda w, k: ((w.hits(k), EXACT),), twin=True),
    Case("label_overlap_hist", [Arg("qlab_packed", I64), Arg("dblab_packed", I64)],
         lambda w, k: {"qlab_packed": w.qlp, "dblab_packed": w.rlp},
         lambda Hm, w, k, a, x: (Hm.label_overlap_hist(a["qlab_packed"], a["dblab_packed"]),),
         lambda w, k: ((w.hist, EXACT),), twin=True),
    Case("ndcg_at_ks", _LIST_ARGS(PITCH) + [Arg("hist", I32, tied=0)], lambda w, k: dict(_lists(w, k), hist=w.hist),
         lambda Hm, w, k, a, x: Hm.ndcg_at_ks(a["idx"], a["qlab_packed"], a["dblab_packed"], KS, hist=a["hist"]),
         lambda w, k: ((w.dcg(KS)[0], DCG), (w.dcg(KS)[1], DCG)), twin=True),
    Case("hamming_map_at_k", _FUSED_ARGS, _fused,
         lambda Hm, w, k, a, x: Hm.hamming_map_at_k(a["q_packed"], x["db"], x["labels"], a["qlab_packed"], w.nbits, k),
         lambda w, k: ((w.ap(k)[0], AP), (w.ap(k)[1], EXACT)), prepare=_prepared),
    Case("hamming_map_at_ks", _FUSED_ARGS, _fused,
         lambda Hm, w, k, a, x: Hm.hamming_map_at_ks(a["q_packed"], x["db"], x["labels"], a["qlab_packed"], w.nbits, KS),
         lambda w, k: ((w.aps(KS)[0], AP), (w.aps(KS)[1], EXACT)), prepare=_prepared),
    Case("hamming_radius_hist", _FUSED_ARGS, _fused,
         lambda Hm, w, k, a, x: Hm.hamming_radius_hist(a["q_packed"], x["db"], x["labels"], a["qlab_packed"], w.nbits),
         lambda w, k: ((w.cum, EXACT), (w.cumrel, EXACT)), twin=True, prepare=_prepared),
    Case("hamming_shard_relbits", _FUSED_ARGS + [Arg("wire", I64, WRITTEN)],
         lambda w, k: dict(_fused(w, k), wire=torch.zeros_like(w.wires[0])),
         lambda Hm, w, k, a, x: (Hm.hamming_shard_relbits(a["q_packed"], x["db"], x["labels"], a["qlab_packed"], w.nbits, SHARD_K,
                                                          wire=a["wire"]).clone(),),
         lambda w, k: ((w.wires[0], EXACT),), shards=True, prepare=_shard0),
    Case("merge_relbits_map", [Arg("wire", I64), Arg("need_out", I32, WRITTEN)],
         lambda w, k: {"wire": w.wires, "need_out": torch.zeros(1, dtype=I32)},
         lambda Hm, w, k, a, x: Hm.merge_relbits_map(a["wire"], SHARD_K, SHARD_K, w.nbits, need_out=a["need_out"]) + (_need(a),),
         lambda w, k: ((w.ap(SHARD_K)[0], AP), (w.ap(SHARD_K)[1], EXACT), (w.need, EXACT)), shards=True),
    Case("merge_relbits_map_ks", [Arg("wire", I64), Arg("need_out", I32, WRITTEN)],
         lambda w, k: {"wire": w.wires, "need_out": torch.zeros(1, dtype=I32)},
         lambda Hm, w, k, a, x: Hm.merge_relbits_map_ks(a["wire"], SHARD_K, KS, w.nbits, need_out=a["need_out"]) + (_need(a),),
         lambda w, k: ((w.aps(KS)[0], AP), (w.aps(KS)[1], EXACT), (w.need, EXACT)), shards=True),
    Case("PreparedDB", [Arg("db_packed", I64)], lambda w, k: {"db_packed": w.rp, "_qp": w.qp}, _prepared_db_call,
         lambda w, k: ((w.rp, EXACT),) + _topk(w, k), twin=True),
    Case("PreparedLabels", [Arg("dblab_packed", I64)], lambda w, k: {"dblab_packed": w.rlp, "_qp": w.qp, "_qlp": w.qlp, "_rp": w.rp},
         _prepared_labels_call, lambda w, k: ((w.rlp, EXACT), (w.cum, EXACT), (w.cumrel, EXACT)), twin=True,
         prepare=lambda Hm, a: {"db": Hm.PreparedDB(a["_rp"])}),
]
PUBLIC = {c.name for c in CASES} - {"hamming_topk_want_cum"}


def runs(twin_only=False):
    """(case, (N, nbits, classes), k) of every row in every world it applies to"""
    out = []
    for case in CASES:
        if twin_only and not case.twin:
            continue
        for cfg in WORLDS:
            if case.shards and cfg[0] != 2 * SHARD_ROWS:
                continue
            for k in ([SHARD_K] if case.shards else [100] if cfg[0] > 257 else [100, cfg[0]]):
                out.append((case, cfg, k))
    return out


def run_id(run):
    case, (N, nbits, classes), k = run
    return f"{case.name}-n{N}-b{nbits}-c{classes}-k{k}"


# ------------------------------------------------------------------------------------------------------------- the forms
def _junk(x):
    """Valid values in other places (rows of other queries or shards): a missed gate reads them and gives a wrong answer,
    never an index outside the database or a count outside a list"""
    return x.flip(0)


def _rows2(x):
    base = torch.empty((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    base[::2], base[1::2] = x, _junk(x)
    return base[::2]


def _cols(x, extra=None):
    extra = x.shape[-1] if extra is None else extra
    return torch.cat([x, _junk(x)[..., :extra]], dim=-1)[..., :x.shape[-1]]


ACCEPTED = {
    "rows2": _rows2,                                                            # rows of a twice-as-tall base
    "cols": _cols,                                                              # column slice of a twice-as-wide base
    "offset": lambda x: torch.cat([_junk(x)[:1], x], dim=0)[1:],                # starts one row into its storage
    "tt": lambda x: x.transpose(-1, -2).contiguous().transpose(-1, -2),         # transposed and back: column-major
    "int64": lambda x: x.long(),                                                # what get_knn hands out
    "pitch": lambda x: _cols(x, min(37, x.shape[-1])),                          # a list prefix, pitch k + 37 (or 2k)
}


def accepted_forms(arg):
    if arg.kind == WRITTEN:
        return []
    return ["rows2", "cols", "offset", "tt"] + (["pitch"] if arg.kind == PITCH else []) + (["int64"] if arg.dtype == INDEX else [])


def make_accepted(form, arg, x):
    """The view of `form` on a base of its own, checked: same values as x, and what a kernel would read from its data_ptr()
    with canonical strides and the declared dtype lies inside the base."""
    v = ACCEPTED[form](x)
    assert v.shape == x.shape and torch.equal(v.to(x.dtype), x)
    if form in ("rows2", "cols", "tt", "pitch") and min(x.shape[-2:]) > 1 and x.shape[0] > 1:
        assert not v.is_contiguous()
    store = v.untyped_storage().nbytes() - v.storage_offset() * v.element_size()
    assert store >= v.numel() * torch.empty((), dtype=arg.declared).element_size()
    return v


NARROW = {I64: I32, I32: I16, I16: torch.int8}
WIDE = {I64: torch.complex128, I32: I64, I16: I32, U8: I32}
FLOAT = {I64: torch.float64, I32: torch.float32, I16: torch.float16, U8: torch.float32}


def refused_forms(arg):
    out = ["float", "rank_up", "device"]
    if arg.declared in NARROW:
        out.append("narrow")
    if arg.dtype != INDEX:                                   # an int64 index list is an accepted form
        out.append("wide")
    if arg.tied is not None:
        out.append("rows")
    if arg.kind == WRITTEN and arg.name != "need_out":       # a one-element tensor is contiguous whatever its stride
        out.append("noncontig")
    if arg.name not in ("need_out", "workspace"):
        out.append("rank_down")
    return out


def make_refused(form, arg, x, foreign):
    """`foreign`: callable moving a tensor to a device the wrapper's module does not take"""
    if form in ("narrow", "wide", "float"):
        return x.to({"narrow": NARROW, "wide": WIDE, "float": FLOAT}[form][arg.declared])
    if form == "rows":
        return x.narrow(arg.tied, 0, x.shape[arg.tied] // 2).contiguous()
    if form == "rank_up":
        return x.unsqueeze(0)
    if form == "rank_down":
        return x.reshape(-1) if x.dim() == 2 else x[0]
    if form == "device":
        return foreign(x)
    if form == "noncontig":
        v = _rows2(x)
        assert not v.is_contiguous()
        return v
    raise KeyError(form)
