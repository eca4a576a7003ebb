"""Host-side Hamming retrieval primitives: the `_cpu` twins of libwvhash.so (csrc/host_rank.cpp) behind the names of
engine/hamming.py, on CPU tensors.  This is the module of the host backend (engine/backend.py): what an explicit device='cpu'
selects in CustomCalculator, RankCache, get_knn, NDCG / ndcg_at / p_topK and the radius metrics -- the configuration the reference itself
runs its calculator in (/root/reference/main/engine/evaluate.py:76-81, accuracy_calculator.py:290-293) and BASELINE config
c0 ("CPU ... plumbing, no GPU").  Same integers as the kernels; average precision bit-identical (same summation order).
No GPU is touched and none is needed.  Every tensor handed to the library passes the gate of engine/_args.py, as in
engine/hamming.py: host tensors only (pack_codes / pack_labels alone move their input here), any stride, int64 index lists
converted, every other dtype or shape mismatch a ValueError."""
import ctypes

import torch

from .. import _lib
from ._args import PITCH, ROWS, anchor, gate

_DEVICE_TYPE = "cpu"             # every tensor argument of this module is a host tensor (_pack alone moves its input here)
_I64, _I32 = torch.int64, torch.int32
SHARD_ROWS_MAX = 1 << 62        # no windowed-kernel limit on the host
MAX_CUTOFFS = 16                # WV_MAX_CUTOFFS


def _words(nbits):
    return (nbits + 63) // 64


def _codes(what, name, t, device=None, words=None, rows=None):
    """Packed int64 rows [rows, words] on the host, gated -> (tensor, device)"""
    device = anchor(t, what, name, _DEVICE_TYPE) if device is None else device
    return gate(t, what, name, _I64, device, (rows, words)), device


def _packed_of(obj, kinds):
    return obj.packed if isinstance(obj, kinds) else obj


def _host(t, dtype=None):
    """_pack's move of whatever it is given to a contiguous host tensor"""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    t = t.detach().cpu()
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous()


def _pack(src, mode, check, what):
    lib = _lib.load()
    src = _host(src, torch.float32)
    if src.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D tensor, got {tuple(src.shape)}")
    src = gate(src, what, "values", torch.float32, src.device, (None, None), PITCH)
    rows, nbits = src.shape
    out = torch.empty((rows, _words(nbits)), dtype=torch.int64)
    flag = ctypes.c_int32(0)
    if rows:
        _lib.check(lib.wv_pack_bits_cpu(_lib.ptr(src), src.stride(0), _lib.ptr(out), rows, nbits, mode,
                                        ctypes.byref(flag) if check else None), "wv_pack_bits_cpu")
    if check and flag.value:
        if mode == 0:
            raise ValueError(f"{what}: codes must be exactly +1/-1 to be bit-packed (found 0, NaN or another value, e.g. sign(0))")
        raise ValueError(f"{what}: labels must be non-negative multi-hot values to be bit-packed")
    return out


def pack_codes(codes, check=True):
    return _pack(codes, 0, check, "pack_codes")


def pack_labels(labels, check=True):
    if labels.dim() == 1:
        raise ValueError("pack_labels: 1-D class-id labels are compared with ==, not packed")
    return _pack(labels, 1, check, "pack_labels")


def bit_counts(packed, nbits):
    lib = _lib.load()
    packed, _ = _codes("bit_counts", "packed", packed, words=_words(nbits))
    counts = torch.empty(nbits, dtype=torch.int32)
    _lib.check(lib.wv_bit_counts_cpu(_lib.ptr(packed), packed.shape[0], nbits, _lib.ptr(counts)), "wv_bit_counts_cpu")
    return counts


def hamming_dist(q_packed, db, nbits=None):
    lib = _lib.load()
    q_packed, dev = _codes("hamming_dist", "q_packed", q_packed)
    db, _ = _codes("hamming_dist", "db", _packed_of(db, PreparedDB), dev)
    Q, words = q_packed.shape
    N = db.shape[0]
    if db.shape[1] != words:
        raise ValueError("hamming_dist: query and database code widths differ")
    nbits = words * 64 if nbits is None else nbits
    if nbits > 255 or _words(nbits) != words:
        raise ValueError(f"hamming_dist: uint8 distances need nbits <= 255 matching the packed width (got nbits={nbits}, {words} words)")
    buf = torch.empty((Q, N), dtype=torch.uint8)
    if Q and N:
        _lib.check(lib.wv_hamming_dist_cpu(_lib.ptr(q_packed), _lib.ptr(db), _lib.ptr(buf), N, Q, N, words), "wv_hamming_dist_cpu")
    return buf


def hamming_topk(q_packed, db, nbits, k, idx_offset=0, workspace=None, want_dist=True, want_cum=False):
    """k nearest database rows per query, ascending (distance, index) -> (idx int32 [Q,k], dist uint8 [Q,k] or None)."""
    if want_cum:
        raise NotImplementedError("hamming_topk on the host: histograms are a by-product of the sharded GPU search only")
    lib = _lib.load()
    q_packed, dev = _codes("hamming_topk", "q_packed", q_packed)
    db, _ = _codes("hamming_topk", "db", _packed_of(db, PreparedDB), dev)
    Q, words = q_packed.shape
    N = db.shape[0]
    if db.shape[1] != words or words != _words(nbits):
        raise ValueError("hamming_topk: code widths do not match nbits")
    idx = torch.empty((Q, k), dtype=torch.int32)
    dist = torch.empty((Q, k), dtype=torch.uint8) if want_dist else None
    if Q:
        _lib.check(lib.wv_hamming_topk_cpu(_lib.ptr(q_packed), _lib.ptr(db), _lib.ptr(idx), _lib.ptr(dist), Q, N, nbits, k,
                                           idx_offset), "wv_hamming_topk_cpu")
    return idx, dist


def _map_at(what, idx, qlab_packed, dblab_packed, k, ks=None):
    from .hamming import _cuts, _columns, _list_args
    lib = _lib.load()
    idx, qlab_packed, dblab_packed, lw = _list_args(what, idx, qlab_packed, dblab_packed, PITCH, _DEVICE_TYPE)
    Q, kfull = idx.shape
    if ks is None:
        k = kfull if k is None else int(k)                  # map_at_k's default: the whole list
    cargs, tail, cols, kmax = _cuts(what, k, ks)
    if not 1 <= kmax <= kfull:
        raise ValueError(f"{what}: cut-off {kmax} outside the lists' length {kfull}")
    ap = torch.empty((Q,) + tail, dtype=torch.float32)
    nrel = torch.empty((Q,) + tail, dtype=torch.int32)
    if Q:
        entry = "wv_map_at_k_cpu" if ks is None else "wv_map_at_ks_cpu"
        _lib.check(getattr(lib, entry)(_lib.ptr(idx), idx.stride(0), Q, *cargs, _lib.ptr(qlab_packed), _lib.ptr(dblab_packed), lw,
                                       _lib.ptr(ap), _lib.ptr(nrel)), entry)
    return _columns(ap, nrel, cols)


def map_at_k(idx, qlab_packed, dblab_packed, k=None):
    return _map_at("map_at_k", idx, qlab_packed, dblab_packed, k)


def map_at_ks(idx, qlab_packed, dblab_packed, ks):
    """map_at_k for several cut-offs from one walk -> (ap float32 [Q, len(ks)], nrel int32 [Q, len(ks)])."""
    return _map_at("map_at_ks", idx, qlab_packed, dblab_packed, None, ks)


def hit_prefix(idx, qlab_packed, dblab_packed):
    from .hamming import _list_args
    lib = _lib.load()
    idx, qlab_packed, dblab_packed, lw = _list_args("hit_prefix", idx, qlab_packed, dblab_packed, ROWS, _DEVICE_TYPE)
    Q, k = idx.shape
    hits = torch.empty((Q, k), dtype=torch.int32)
    if Q:
        _lib.check(lib.wv_hit_prefix_cpu(_lib.ptr(idx), Q, k, _lib.ptr(qlab_packed), _lib.ptr(dblab_packed), lw, _lib.ptr(hits)),
                   "wv_hit_prefix_cpu")
    return hits


class PreparedDB:
    """Nothing to prepare on the host: keeps the packed codes (the calculator's code path is shared with the GPU)."""

    def __init__(self, db_packed, nbits=None, _virtual=True):
        self.packed, _ = _codes("PreparedDB", "db_packed", db_packed)
        self.N, self.words = self.packed.shape
        self.nbits = nbits if nbits is not None else self.words * 64
        self.parts = None


class PreparedLabels:
    """Nothing to prepare on the host either: keeps the packed label words."""

    def __init__(self, dblab_packed):
        self.packed, _ = _codes("PreparedLabels", "dblab_packed", dblab_packed)
        self.N, self.words = self.packed.shape
        self.parts, self.ok, self.blob = None, self.words <= 2, None


def hamming_radius_hist(q_packed, db, labels, qlab_packed, nbits):
    """hamming.hamming_radius_hist through the host twin (wv_hamming_radius_hist_cpu), any N -> (cum, cumrel) int32
    [Q, nbits + 2], the kernel's integers.  db / labels: PreparedDB / PreparedLabels of this module or packed int64 tensors."""
    lib = _lib.load()
    what = "hamming_radius_hist"
    q_packed, dev = _codes(what, "q_packed", q_packed)
    Q, words = q_packed.shape
    qlab_packed, _ = _codes(what, "qlab_packed", qlab_packed, dev, rows=Q)
    dbp, _ = _codes(what, "db", _packed_of(db, PreparedDB), dev)
    lab, _ = _codes(what, "labels", _packed_of(labels, PreparedLabels), dev)
    if dbp.shape[1] != words or lab.shape[0] != dbp.shape[0] or words != _words(nbits):
        raise ValueError("hamming_radius_hist: query / database / label shapes disagree")
    if lab.shape[1] > 2 or qlab_packed.shape[1] != lab.shape[1] or nbits > 128:
        return None
    cum = torch.zeros((Q, nbits + 2), dtype=torch.int32)
    cumrel = torch.zeros_like(cum)
    if Q and dbp.shape[0]:                           # an empty shard contributes zeros
        _lib.check(lib.wv_hamming_radius_hist_cpu(_lib.ptr(q_packed), _lib.ptr(dbp), _lib.ptr(qlab_packed), _lib.ptr(lab), lab.shape[1],
                                                  Q, dbp.shape[0], nbits, _lib.ptr(cum), _lib.ptr(cumrel)), "wv_hamming_radius_hist_cpu")
    return cum, cumrel


def label_overlap_hist(qlab_packed, dblab_packed):
    """hamming.label_overlap_hist through the host twin (wv_label_overlap_hist_cpu): the same integers."""
    from .hamming import _graded_words, _label_args
    lib = _lib.load()
    dev = anchor(qlab_packed, "label_overlap_hist", "qlab_packed", _DEVICE_TYPE)
    qlab_packed, dblab_packed, lw = _label_args("label_overlap_hist", qlab_packed, dblab_packed, None, dev)
    _graded_words(lw, "label_overlap_hist")
    Q, N = qlab_packed.shape[0], dblab_packed.shape[0]
    hist = torch.zeros((Q, 64 * lw + 1), dtype=torch.int32)
    if Q and N:
        _lib.check(lib.wv_label_overlap_hist_cpu(_lib.ptr(qlab_packed), _lib.ptr(dblab_packed), lw, Q, N, _lib.ptr(hist)),
                   "wv_label_overlap_hist_cpu")
    return hist


def ndcg_at_ks(idx, qlab_packed, dblab_packed, ks, hist=None):
    """hamming.ndcg_at_ks through the host twin (wv_ndcg_at_ks_cpu): the same table w, the same summation order, the
    kernel's bits -> (dcg, idcg) float64 [Q, len(ks)]."""
    from .hamming import _cutoffs, _columns, _graded_words, _list_args, ndcg_weights
    lib = _lib.load()
    idx, qlab_packed, dblab_packed, lw = _list_args("ndcg_at_ks", idx, qlab_packed, dblab_packed, PITCH, _DEVICE_TYPE)
    _graded_words(lw, "ndcg_at_ks")
    Q, kfull = idx.shape
    uniq, c_ks, cols = _cutoffs(ks, "ndcg_at_ks")
    if uniq[-1] > kfull:
        raise ValueError(f"ndcg_at_ks: cut-off {uniq[-1]} outside the lists' length {kfull}")
    if hist is None:
        hist = label_overlap_hist(qlab_packed, dblab_packed)
    hist = gate(hist, "ndcg_at_ks", "hist (the int32 [Q, 64 * lwords + 1] table of label_overlap_hist)", _I32, idx.device, (Q, 64 * lw + 1))
    w = ndcg_weights(uniq[-1])
    dcg = torch.zeros((Q, len(uniq)), dtype=torch.float64)
    idcg = torch.zeros_like(dcg)
    if Q:
        _lib.check(lib.wv_ndcg_at_ks_cpu(_lib.ptr(idx), idx.stride(0), Q, c_ks, len(uniq), _lib.ptr(qlab_packed), _lib.ptr(dblab_packed),
                                         lw, _lib.ptr(hist), _lib.ptr(w), _lib.ptr(dcg), _lib.ptr(idcg)), "wv_ndcg_at_ks_cpu")
    return _columns(dcg, idcg, cols)


IP_MAP_ROWS_MAX = _lib.WV_IP_MAP_ROWS_MAX


def ip_map_at_k(q, db, qlab_packed, dblab_packed, k):
    """hamming.ip_map_at_k through the host twin (wv_ip_map_at_k_cpu): the kernel's bits, the same limits -> (ap float32 [Q],
    nrel int32 [Q]) or None outside them."""
    from .hamming import _ip_map_args
    lib = _lib.load()
    q, db, qlab_packed, dblab_packed, lw, k = _ip_map_args("ip_map_at_k", q, db, qlab_packed, dblab_packed, k, _DEVICE_TYPE)
    if lw > 2:
        return None
    Q = q.shape[0]
    ap, nrel = torch.empty(Q, dtype=torch.float32), torch.empty(Q, dtype=torch.int32)
    if not Q:
        return ap, nrel
    rc = lib.wv_ip_map_at_k_cpu(_lib.ptr(q), _lib.ptr(db), Q, db.shape[0], q.shape[1], _lib.ptr(qlab_packed), _lib.ptr(dblab_packed),
                                lw, k, _lib.ptr(ap), _lib.ptr(nrel))
    if rc == _lib.WV_ENOTSUP:
        return None
    _lib.check(rc, "wv_ip_map_at_k_cpu")
    return ap, nrel


def hamming_map_at_k(*args, **kwargs):
    return None                   # ranking and AP are two calls on the host (same numbers)


def hamming_map_at_ks(*args, **kwargs):
    return None
