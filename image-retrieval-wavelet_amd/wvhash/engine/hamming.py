"""Device-side Hamming retrieval primitives (thin wrappers over the C ABI, include/wvhash.h).

Codes are +-1 fp32 rows in the reference (torch.sign output, multi_dino_attention.py:833); here
they are packed 64 per int64 word once and stay on the GPU.
"""
import ctypes

import torch

from .. import _lib
from ._args import INDEX, PITCH, ROWS, WRITTEN, anchor, gate, same_device

_DEVICE_TYPE = "cuda"            # where every tensor argument of this module lives (_pack alone moves its input there)
_I64, _I32, _I16, _U8 = torch.int64, torch.int32, torch.int16, torch.uint8


def _words(nbits):
    return (nbits + 63) // 64


def _pack(src, mode, check, what):
    lib = _lib.require_gpu()
    if src.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D tensor, got {tuple(src.shape)}")
    src = src.to(device=_device_of(src), dtype=torch.float32)       # the one wrapper that moves and converts what it is given
    src = gate(src, what, "values", torch.float32, src.device, (None, None), PITCH)
    rows, nbits = src.shape
    out = torch.empty((rows, _words(nbits)), dtype=torch.int64, device=src.device)
    flag = torch.zeros(1, dtype=torch.int32, device=src.device) if check else None
    if rows:
        with torch.cuda.device(src.device):
            rc = lib.wv_pack_bits(_lib.ptr(src), src.stride(0), _lib.ptr(out), rows, nbits, mode,
                                  _lib.ptr(flag), _lib.stream_ptr())
            _lib.check(rc, "wv_pack_bits")
    if check and rows and int(flag.item()):
        if mode == 0:
            raise ValueError(f"{what}: codes must be exactly +1/-1 to be bit-packed (found 0, NaN or another "
                             "value, e.g. sign(0)); use the float path get_knn(..., distance_metric='cosine')")
        raise ValueError(f"{what}: labels must be non-negative multi-hot values to be bit-packed")
    return out


def _device_of(t):
    if t.is_cuda:
        return t.device
    _lib.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def pack_codes(codes, check=True):
    """[N, nbits] +-1 -> int64 [N, ceil(nbits/64)], bit j of word w = codes[:, 64w+j] > 0."""
    return _pack(codes, 0, check, "pack_codes")


def pack_labels(labels, check=True):
    """[N, Lc] multi-hot (>= 0) -> int64 [N, ceil(Lc/64)]."""
    if labels.dim() == 1:
        raise ValueError("pack_labels: 1-D class-id labels are compared with ==, not packed")
    return _pack(labels, 1, check, "pack_labels")


def bit_counts(packed, nbits):
    lib = _lib.require_gpu()
    packed = gate(packed, "bit_counts", "packed", _I64, anchor(packed, "bit_counts", "packed", _DEVICE_TYPE), (None, _words(nbits)))
    counts = torch.empty(nbits, dtype=torch.int32, device=packed.device)
    with torch.cuda.device(packed.device):
        rc = lib.wv_bit_counts(_lib.ptr(packed), packed.shape[0], nbits, _lib.ptr(counts), _lib.stream_ptr())
        _lib.check(rc, "wv_bit_counts")
    return counts


SHARD_ROWS_MAX = 32768      # wv_hamming_hist / wv_hamming_topk_rows16 take shards up to this many rows
MAX_CUTOFFS = 16            # WV_MAX_CUTOFFS: different cut-offs one multi-k call takes
RANK_K_MAX = 32639          # longest list the windowed kernel builds (its 16-bit cells count list bytes: 2 (k + 128) < 65536)


class PreparedDB:
    """A packed database laid out once for the kernels (wv_db_prepare): what index.add() is to the
    reference's faiss path (get_knn.py:54), except that it is built once per database, not per call."""

    def __init__(self, db_packed, nbits=None, _virtual=True):
        lib = _lib.require_gpu()
        self.packed = gate(db_packed, "PreparedDB", "db_packed (packed int64 codes [N, words], see pack_codes)", _I64,
                           anchor(db_packed, "PreparedDB", "db_packed", _DEVICE_TYPE), (None, None))
        self.N, self.words = self.packed.shape
        self.nbits = nbits if nbits is not None else self.words * 64
        nbytes = lib.wv_db_prepared_bytes(self.N, self.words)
        self.blob = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.packed.device)
        if self.N:
            with torch.cuda.device(self.packed.device):
                rc = lib.wv_db_prepare(_lib.ptr(self.packed), self.N, self.words, _lib.ptr(self.blob),
                                       ctypes.c_size_t(nbytes), _lib.stream_ptr())
                _lib.check(rc, "wv_db_prepare")
        # A database beyond the windowed ranking kernel's 32,768 rows is ranked as contiguous VIRTUAL shards on the one
        # GPU (the row-sharded search of wvhash/parallel.py without the collectives: histograms -> prefix length ->
        # 16-bit list prefixes -> merge): 117,218 x 128-bit codes, 5000 queries, k = 5000: 1.1 ms instead of 1.83 ms for
        # the first-generation kernel.
        self.parts, self.per = None, None
        if SHARD_ROWS_MAX < self.N <= 64 * SHARD_ROWS_MAX and self.words <= 2 and _virtual:
            g = -(-self.N // SHARD_ROWS_MAX)
            self.per = -(-self.N // g)
            self.parts = [PreparedDB(self.packed[lo:min(self.N, lo + self.per)], self.nbits, _virtual=False)
                          for lo in range(0, self.N, self.per)]

    @property
    def shape(self):
        return self.packed.shape

    @property
    def device(self):
        return self.packed.device


def _db_arg(what, db, device):
    """`db` of the ranking wrappers: a PreparedDB on the anchor device or packed int64 codes [N, words]
    -> (prepared, the PreparedDB or the gated tensor, N, words)"""
    if isinstance(db, PreparedDB):
        same_device(db, what, "db", device)
        return True, db, db.N, db.words
    db = gate(db, what, "db", _I64, device, (None, None))
    return False, db, db.shape[0], db.shape[1]


def hamming_dist(q_packed, db, nbits=None):
    """-> uint8 [Q, N] view (row pitch padded to 64 bytes so every row store is 16-B aligned).
    `db`: packed int64 codes [N, words] or a PreparedDB.  Distances are bytes: codes of more than 255 bits could
    reach 256 (complementary codes), which would wrap to 0 -- refused; `nbits` tells a 193..255-bit code
    (4 words, fine) from a 256-bit one."""
    lib = _lib.require_gpu()
    dev = anchor(q_packed, "hamming_dist", "q_packed", _DEVICE_TYPE)
    q_packed = gate(q_packed, "hamming_dist", "q_packed", _I64, dev, (None, None))
    Q, words = q_packed.shape
    prepared, db, N, dwords = _db_arg("hamming_dist", db, dev)
    if dwords != words:
        raise ValueError("hamming_dist: query and database code widths differ")
    if nbits is None:
        nbits = db.nbits if prepared else words * 64
    if nbits > 255 or _words(nbits) != words:
        raise ValueError(f"hamming_dist: uint8 distances need nbits <= 255 matching the packed width "
                         f"(got nbits={nbits}, {words} words); pass nbits for 193..255-bit codes")
    ld = (N + 63) // 64 * 64
    buf = torch.empty((Q, ld), dtype=torch.uint8, device=q_packed.device)
    if Q and N:
        with torch.cuda.device(q_packed.device):
            if prepared:
                rc = lib.wv_hamming_dist_prepared(_lib.ptr(q_packed), _lib.ptr(db.blob), _lib.ptr(buf), ld, Q, N,
                                                  words, _lib.stream_ptr())
            else:
                rc = lib.wv_hamming_dist(_lib.ptr(q_packed), _lib.ptr(db), _lib.ptr(buf), ld, Q, N, words,
                                         _lib.stream_ptr())
            _lib.check(rc, "wv_hamming_dist")
    return buf[:, :N]


class TopkWorkspace:
    """Reusable scratch for hamming_topk (the transposed database image)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return self.buf


def hamming_topk(q_packed, db, nbits, k, idx_offset=0, workspace=None, want_dist=True, want_cum=False):
    """k nearest database rows per query, ascending (distance, index).
    `db`: packed int64 codes [N, words] or a PreparedDB.
    -> (idx int32 [Q,k], dist uint8 [Q,k] or None)   [+ cum int32 [Q, nbits+2] when want_cum:
    cum[q, b] = number of rows with distance < b]."""
    lib = _lib.require_gpu()
    dev = anchor(q_packed, "hamming_topk", "q_packed", _DEVICE_TYPE)
    q_packed = gate(q_packed, "hamming_topk", "q_packed", _I64, dev, (None, None))
    Q, words = q_packed.shape
    prepared, db, N = _shard_db_args(db, words, nbits, "hamming_topk", dev)
    if prepared and db.parts and not want_cum and nbits <= 128 and Q:
        got = _virtual_shards_topk(q_packed, db, nbits, k, idx_offset, want_dist)
        if got is not None:                                 # None: a prefix beyond the windowed kernel's lists -- rank the whole database
            return got
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    dist = torch.empty((Q, k), dtype=torch.uint8, device=dev) if want_dist else None
    cum = torch.empty((Q, nbits + 2), dtype=torch.int32, device=dev) if want_cum else None
    blob = db.blob if prepared and words <= 2 else None     # the ranking images exist for codes of <= 2 words
    ws = None
    if blob is None:                                        # the kernel's image of the database is made per call
        ws = _workspace("hamming_topk", workspace, lib.wv_hamming_topk_workspace_bytes(Q, N, words, k), dev)
    with torch.cuda.device(dev):
        rc = lib.wv_hamming_topk_ex(_lib.ptr(q_packed), _lib.ptr(db.packed if prepared else db), _lib.ptr(blob), _lib.ptr(idx),
                                    _lib.ptr(dist), _lib.ptr(cum), Q, N, nbits, k, idx_offset, _lib.ptr(ws),
                                    ctypes.c_size_t(ws.numel() if ws is not None else 0), _lib.stream_ptr())
        _lib.check(rc, "wv_hamming_topk_ex")
    return (idx, dist, cum) if want_cum else (idx, dist)


def owed_prefix(cum, cum_total, k):
    """The prefix rule of the sharded search.  cum int32 [..., Q, nbits + 2]: cumulative distance histograms of one shard or of
    several; cum_total [Q, nbits + 2]: their sum over ALL shards of the database.  A query's global k-th distance T is the
    first bin b with cum_total[q, b + 1] >= k (rows of the whole database with distance <= b); a shard owes the query its
    cum[q, T + 1] rows with distance <= T.
    -> int32 [1] on the histograms' device: the longest prefix any of these shards owes any query.  No host read."""
    T = (cum_total[:, 1:] >= k).int().argmax(dim=1)
    return torch.gather(cum, -1, (T + 1).unsqueeze(1).expand(*cum.shape[:-1], 1)).max().reshape(1)


def _virtual_prefix(q_packed, db, nbits, k):
    """First step of every virtual-shard route: the parts' histograms and the prefix length each part contributes (one host
    read, as in the un-hinted sharded search) -> (cums int32 [G, Q, nbits + 2], send)."""
    cums = torch.stack([hamming_hist(q_packed, part, nbits) for part in db.parts])
    return cums, max(1, min(k, db.per, int(owed_prefix(cums, cums.sum(0), k).item())))


def _virtual_shards_topk(q_packed, db, nbits, k, idx_offset, want_dist):
    cums, send = _virtual_prefix(q_packed, db, nbits, k)
    if send > RANK_K_MAX:
        return None
    Q = q_packed.shape[0]
    lists = torch.zeros((len(db.parts), Q, send), dtype=torch.int16, device=q_packed.device)
    for g, part in enumerate(db.parts):
        w = min(send, part.N)
        lists[g, :, :w] = hamming_topk_rows16(q_packed, part, nbits, w)
    idx, dist = topk_merge_cum(lists, cums, db.per, k, nbits)
    if idx_offset:
        idx += int(idx_offset)
    return idx, (dist if want_dist else None)


def _shard_db_args(db, words, nbits, what, device):
    prepared, db, N, dwords = _db_arg(what, db, device)
    if dwords != words or words != _words(nbits):
        raise ValueError(f"{what}: code widths do not match nbits")
    return prepared, db, N


def _workspace(what, workspace, nbytes, device):
    """The scratch of a call on an unprepared database: the caller's TopkWorkspace (grown as needed) or one for this call.
    A buffer the caller's workspace already holds is written as it stands: bytes, contiguous, on the anchor device."""
    workspace = workspace or TopkWorkspace()
    if workspace.buf is not None:
        gate(workspace.buf, what, "workspace", _U8, device, (None,), WRITTEN)
    return gate(workspace.get(nbytes, device), what, "workspace", _U8, device, (None,), WRITTEN)


def _shard_step(what, q_packed, db, nbits, k, workspace, want_rows, want_cum):
    """One call of the sharded search's kernel on one shard -> (rows int16 [Q, k] or None, cum int32 [Q, nbits + 2] or None)."""
    lib = _lib.require_gpu()
    dev = anchor(q_packed, what, "q_packed", _DEVICE_TYPE)
    q_packed = gate(q_packed, what, "q_packed", _I64, dev, (None, None))
    Q, words = q_packed.shape
    prepared, db, N = _shard_db_args(db, words, nbits, what, dev)
    rows = torch.empty((Q, k), dtype=torch.int16, device=dev) if want_rows else None
    cum = torch.empty((Q, nbits + 2), dtype=torch.int32, device=dev) if want_cum else None
    ws = None
    if not prepared:
        ws = _workspace(what, workspace, lib.wv_hamming_topk_workspace_bytes(Q, N, words, max(k, 1)), dev)
    src = (None if prepared else _lib.ptr(db), _lib.ptr(db.blob) if prepared else None)
    tail = (_lib.ptr(ws), ctypes.c_size_t(ws.numel() if ws is not None else 0), _lib.stream_ptr())
    with torch.cuda.device(dev):
        if not want_rows:
            rc = lib.wv_hamming_hist(_lib.ptr(q_packed), *src, _lib.ptr(cum), Q, N, nbits, *tail)
        elif not want_cum:
            rc = lib.wv_hamming_topk_rows16(_lib.ptr(q_packed), *src, _lib.ptr(rows), Q, N, nbits, k, *tail)
        else:
            rc = lib.wv_hamming_shard_prefix(_lib.ptr(q_packed), *src, _lib.ptr(rows), _lib.ptr(cum), Q, N, nbits, k, *tail)
        _lib.check(rc, "wv_" + what)
    return rows, cum


def hamming_hist(q_packed, db, nbits, workspace=None):
    """Cumulative distance histogram of every query over the rows of `db` (no list is built):
    cum int32 [Q, nbits + 2], cum[q, b] = rows with distance < b.  First step of the sharded search."""
    return _shard_step("hamming_hist", q_packed, db, nbits, 0, workspace, False, True)[1]


def hamming_topk_rows16(q_packed, db, nbits, k, workspace=None):
    """The k nearest rows of `db` per query, ascending (distance, row), as 16-bit LOCAL row numbers (int16 storage of
    uint16 values [Q, k]): the wire format of the sharded search (topk_merge_cum)."""
    return _shard_step("hamming_topk_rows16", q_packed, db, nbits, k, workspace, True, False)[0]


def hamming_shard_prefix(q_packed, db, nbits, k, workspace=None):
    """hamming_topk_rows16 and hamming_hist in one pass -> (rows int16 [Q, k], cum int32 [Q, nbits + 2])."""
    return _shard_step("hamming_shard_prefix", q_packed, db, nbits, k, workspace, True, True)


def topk_merge(idx_in, dist_in, k, nbits):
    """[G,Q,kin] per-shard lists (contiguous row shards in rank order) -> global [Q,k]."""
    lib = _lib.require_gpu()
    dev = anchor(idx_in, "topk_merge", "idx_in", _DEVICE_TYPE)
    idx_in = gate(idx_in, "topk_merge", "idx_in", INDEX, dev, (None, None, None))
    G, Q, kin = idx_in.shape
    dist_in = gate(dist_in, "topk_merge", "dist_in", _U8, dev, (G, Q, kin))
    idx = torch.empty((Q, k), dtype=torch.int32, device=idx_in.device)
    dist = torch.empty((Q, k), dtype=torch.uint8, device=idx_in.device)
    with torch.cuda.device(idx_in.device):
        rc = lib.wv_topk_merge(_lib.ptr(idx_in), _lib.ptr(dist_in), G, Q, kin, _lib.ptr(idx), _lib.ptr(dist), k,
                               nbits, _lib.stream_ptr())
        _lib.check(rc, "wv_topk_merge")
    return idx, dist


def topk_merge_cum(idx_local, cum, shard_rows, k, nbits, need_out=None):
    """Compact merge: idx_local int16 storage of uint16 LOCAL row numbers [G,Q,kin], cum int32 [G,Q,nbits+2]
    (per-shard cumulative distance histograms) -> global (idx int32 [Q,k], dist uint8 [Q,k]).
    need_out: int32 [1] device tensor (zeroed by the caller) that receives the longest prefix any shard had to contribute
    for any of these queries -- the lists are exact iff it is <= kin."""
    lib = _lib.require_gpu()
    dev = anchor(idx_local, "topk_merge_cum", "idx_local", _DEVICE_TYPE)
    idx_local = gate(idx_local, "topk_merge_cum", "idx_local", _I16, dev, (None, None, None))
    G, Q, kin = idx_local.shape
    cum = gate(cum, "topk_merge_cum", "cum", _I32, dev, (G, Q, nbits + 2))
    if need_out is not None:
        need_out = gate(need_out, "topk_merge_cum", "need_out", _I32, dev, (1,), WRITTEN)
    idx = torch.empty((Q, k), dtype=torch.int32, device=idx_local.device)
    dist = torch.empty((Q, k), dtype=torch.uint8, device=idx_local.device)
    with torch.cuda.device(idx_local.device):
        rc = lib.wv_topk_merge_cum_need(_lib.ptr(idx_local), _lib.ptr(cum), G, Q, kin, shard_rows, _lib.ptr(idx),
                                        _lib.ptr(dist), k, nbits, _lib.ptr(need_out),
                                        _lib.stream_ptr())
        _lib.check(rc, "wv_topk_merge_cum_need")
    return idx, dist


def rank_from_dist(dist_matrix, nbits, k):
    lib = _lib.require_gpu()
    dist_matrix = gate(dist_matrix, "rank_from_dist", "dist_matrix", _U8, anchor(dist_matrix, "rank_from_dist", "dist_matrix", _DEVICE_TYPE),
                       (None, None), PITCH)
    Q, N = dist_matrix.shape
    idx = torch.empty((Q, k), dtype=torch.int32, device=dist_matrix.device)
    dist = torch.empty((Q, k), dtype=torch.uint8, device=dist_matrix.device)
    with torch.cuda.device(dist_matrix.device):
        rc = lib.wv_rank_from_dist(_lib.ptr(dist_matrix), dist_matrix.stride(0), Q, N, nbits, _lib.ptr(idx),
                                   _lib.ptr(dist), k, _lib.stream_ptr())
        _lib.check(rc, "wv_rank_from_dist")
    return idx, dist


def _cuts(what, k, ks):
    """Where a single-k entry point and its multi-k twin differ: k is one cut-off (ks None) or ks holds several, as they
    arrive -> (the C arguments that stand where k stands, trailing shape of ap / nrel, column of every requested cut-off or
    None, largest cut-off)."""
    if ks is None:
        return (k,), (), None, k
    uniq, c_ks, cols = _cutoffs(ks, what)
    return (c_ks, len(uniq)), (len(uniq),), cols, uniq[-1]


def _ap_buffers(Q, tail, device):
    return torch.empty((Q,) + tail, dtype=torch.float32, device=device), torch.empty((Q,) + tail, dtype=torch.int32, device=device)


def _list_args(what, idx, qlab_packed, dblab_packed, kind, device_type=None):
    """The arguments of the wrappers that walk ranked lists: idx [Q, k] (int32; int64 is converted), one row of packed label
    words per list, the database rows' label words of the same width -> (idx, qlab_packed, dblab_packed, label words), gated."""
    dev = anchor(idx, what, "idx", device_type or _DEVICE_TYPE)
    idx = gate(idx, what, "idx", INDEX, dev, (None, None), kind)
    qlab_packed, dblab_packed, lw = _label_args(what, qlab_packed, dblab_packed, idx.shape[0], dev)
    return idx, qlab_packed, dblab_packed, lw


def _label_args(what, qlab_packed, dblab_packed, Q, dev):
    qlab_packed = gate(qlab_packed, what, "qlab_packed", _I64, dev, (Q, None))
    dblab_packed = gate(dblab_packed, what, "dblab_packed", _I64, dev, (None, None))
    if dblab_packed.shape[1] != qlab_packed.shape[1]:
        raise ValueError(f"{what}: label widths differ")
    return qlab_packed, dblab_packed, qlab_packed.shape[1]


def _map_at(what, idx, qlab_packed, dblab_packed, k, ks=None):
    lib = _lib.require_gpu()
    idx, qlab_packed, dblab_packed, lw = _list_args(what, idx, qlab_packed, dblab_packed, PITCH)
    Q, kfull = idx.shape
    if ks is None:
        k = kfull if k is None else int(k)                  # map_at_k's default: the whole list
    cargs, tail, cols, kmax = _cuts(what, k, ks)
    if not 1 <= kmax <= kfull:
        raise ValueError(f"{what}: cut-off {kmax} outside the lists' length {kfull}")
    ap, nrel = _ap_buffers(Q, tail, idx.device)
    if Q:
        entry = "wv_map_at_k_ld" if ks is None else "wv_map_at_ks"
        with torch.cuda.device(idx.device):
            rc = getattr(lib, entry)(_lib.ptr(idx), idx.stride(0), Q, *cargs, _lib.ptr(qlab_packed), _lib.ptr(dblab_packed), lw,
                                     _lib.ptr(ap), _lib.ptr(nrel), _lib.stream_ptr())
            _lib.check(rc, entry)
    return _columns(ap, nrel, cols)


def map_at_k(idx, qlab_packed, dblab_packed, k=None):
    """Average precision per query over (the first k entries of) its ranked list -> (ap float32 [Q], nrel int32 [Q]).
    idx: int32 [Q, >= k] (int64 is converted; a prefix idx[:, :k'] of wider lists is read in place); qlab_packed: int64
    [Q, words], one row per list.  The VALUES of idx are not checked against the rows of dblab_packed: the entry point carries
    no N, and a check would cost a reduction and a host read per call."""
    return _map_at("map_at_k", idx, qlab_packed, dblab_packed, k)


def map_at_ks(idx, qlab_packed, dblab_packed, ks):
    """map_at_k for several cut-offs from ONE pass over the lists (read once, labels gathered once)
    -> (ap float32 [Q, len(ks)], nrel int32 [Q, len(ks)]), column i = map_at_k(idx, ..., k=ks[i])."""
    return _map_at("map_at_ks", idx, qlab_packed, dblab_packed, None, ks)


class PreparedLabels:
    """The database rows' packed label words laid out for the fused ranking + AP kernel (wv_rank_labels_prepare): one
    or two 64-bit multi-hot words per row (up to 128 classes), databases of at most 32,768 rows.  `ok` is False for anything else -- the caller then
    ranks and evaluates in two steps."""

    def __init__(self, dblab_packed, _virtual=True):
        lib = _lib.require_gpu()
        self.packed = gate(dblab_packed, "PreparedLabels", "dblab_packed (packed int64 label words [N, words], see pack_labels)", _I64,
                           anchor(dblab_packed, "PreparedLabels", "dblab_packed", _DEVICE_TYPE), (None, None))
        self.N, self.words = self.packed.shape
        self.parts = None
        if SHARD_ROWS_MAX < self.N <= 64 * SHARD_ROWS_MAX and self.words <= 2 and _virtual:      # as PreparedDB: virtual shards
            g = -(-self.N // SHARD_ROWS_MAX)
            per = -(-self.N // g)
            self.parts = [PreparedLabels(self.packed[lo:min(self.N, lo + per)], _virtual=False) for lo in range(0, self.N, per)]
        nbytes = lib.wv_rank_labels_prepared_bytes(self.N, self.words) if self.words <= 2 and self.N and not self.parts else 0
        self.ok = nbytes > 0 or bool(self.parts)
        self.blob = None
        if nbytes:
            self.blob = torch.empty(nbytes, dtype=torch.uint8, device=self.packed.device)
            with torch.cuda.device(self.packed.device):
                rc = lib.wv_rank_labels_prepare(_lib.ptr(self.packed), self.N, self.words, _lib.ptr(self.blob), ctypes.c_size_t(nbytes),
                                                _lib.stream_ptr())
                _lib.check(rc, "wv_rank_labels_prepare")


def _fused_gate(what, q_packed, db, labels, qlab_packed, nbits, code_width=False):
    """The argument check of the entry points that read codes and labels in one kernel.  TypeError for unprepared inputs,
    ValueError for shapes that disagree (code_width: the packed width must also be nbits'); -> False when the shape is outside
    the fused kernels (labels wider than 2 words, nbits > 128): the caller answers None.
    -> (inside the fused kernels, q_packed, qlab_packed), the two tensors gated: int64 rows on one device with `db` and `labels`,
    one row of label words per query."""
    if not isinstance(db, PreparedDB) or not isinstance(labels, PreparedLabels):
        raise TypeError(f"{what}: needs a PreparedDB and PreparedLabels")
    dev = anchor(q_packed, what, "q_packed", _DEVICE_TYPE)
    q_packed = gate(q_packed, what, "q_packed", _I64, dev, (None, None))
    qlab_packed = gate(qlab_packed, what, "qlab_packed", _I64, dev, (q_packed.shape[0], None))
    same_device(db, what, "db", dev)
    same_device(labels, what, "labels", dev)
    words = q_packed.shape[1]
    if words != db.words or labels.N != db.N or (code_width and words != _words(nbits)):
        raise ValueError(f"{what}: query / database / label shapes disagree")
    return labels.ok and qlab_packed.shape[1] == labels.words and nbits <= 128, q_packed, qlab_packed


def _fused_map(what, q_packed, db, labels, qlab_packed, nbits, k, ks=None):
    """hamming_map_at_k (ks None) and hamming_map_at_ks: gate, virtual-shard route, direct route; the leaves differ (_cuts)."""
    lib = _lib.require_gpu()
    ok, q_packed, qlab_packed = _fused_gate(what, q_packed, db, labels, qlab_packed, nbits)
    cargs, tail, cols, kmax = _cuts(what, k, ks)
    if ks is not None and kmax > db.N:
        raise ValueError(f"{what}: largest cut-off {kmax} must be <= N={db.N}")
    if not ok or not 1 <= kmax <= db.N:
        return None
    Q = q_packed.shape[0]
    dev = q_packed.device
    if db.parts or labels.parts:                         # more than 32,768 rows: virtual shards, relevance strings, one merge
        if not (db.parts and labels.parts) or len(db.parts) != len(labels.parts) or not Q:
            return None
        send = _virtual_prefix(q_packed, db, nbits, kmax)[1]     # one prefix length, for the largest cut-off
        if send > RANK_K_MAX:
            return None
        wires = torch.zeros((len(db.parts), Q, relbits_wire_words(send, nbits)), dtype=torch.int64, device=dev)
        for g, (part, lab) in enumerate(zip(db.parts, labels.parts)):
            if hamming_shard_relbits(q_packed, part, lab, qlab_packed, nbits, min(send, part.N), wire=wires[g], kin=send) is None:
                return None
        return merge_relbits_map(wires, send, k, nbits) if ks is None else merge_relbits_map_ks(wires, send, ks, nbits)
    ap, nrel = _ap_buffers(Q, tail, dev)
    if Q:
        with torch.cuda.device(dev):
            rc = getattr(lib, "wv_" + what)(_lib.ptr(q_packed), _lib.ptr(db.blob), _lib.ptr(labels.blob),
                                            _lib.ptr(qlab_packed), labels.words, Q, db.N, nbits, *cargs, _lib.ptr(ap),
                                            _lib.ptr(nrel), _lib.stream_ptr())
            if rc == _lib.WV_ENOTSUP:
                return None
            _lib.check(rc, "wv_" + what)
    return _columns(ap, nrel, cols)


def hamming_map_at_k(q_packed, db, labels, qlab_packed, nbits, k):
    """mAP@k ingredients straight from the codes -> (ap float32 [Q], nrel int32 [Q]), or None when the shape is outside
    the fused kernel (the caller then runs hamming_topk + map_at_k, which return exactly the same numbers).
    db: PreparedDB; labels: PreparedLabels of the same rows; qlab_packed: int64 [Q, 1 or 2]."""
    return _fused_map("hamming_map_at_k", q_packed, db, labels, qlab_packed, nbits, k)


def hamming_map_at_ks(q_packed, db, labels, qlab_packed, nbits, ks):
    """hamming_map_at_k for several cut-offs from ONE ranking pass -> (ap float32 [Q, len(ks)], nrel int32 [Q, len(ks)]),
    column i = what hamming_map_at_k returns for k = ks[i]; or None when the largest cut-off is outside the fused kernel
    (the caller then runs hamming_topk at max(ks) + map_at_ks: the same numbers).  ks: any order, repeats allowed, at most
    MAX_CUTOFFS different values."""
    return _fused_map("hamming_map_at_ks", q_packed, db, labels, qlab_packed, nbits, None, ks)


IP_MAP_ROWS_MAX = _lib.WV_IP_MAP_ROWS_MAX     # WV_IP_MAP_ROWS_MAX: rows wv_ip_map_at_k ranks inside one workgroup


def _ip_map_args(what, q, db, qlab_packed, dblab_packed, k, device_type):
    """The arguments of ip_map_at_k on either side: fp32 rows on one device (bf16 / fp16 embeddings are widened, which is
    exact), one row of packed label words per embedding row -> (q, db, qlab_packed, dblab_packed, label words, k), gated."""
    dev = anchor(q, what, "q", device_type)
    q, db = (t.float() if torch.is_tensor(t) and t.dtype in (torch.bfloat16, torch.float16) else t for t in (q, db))
    q = gate(q, what, "q", torch.float32, dev, (None, None))
    db = gate(db, what, "db", torch.float32, dev, (None, q.shape[1]))
    qlab_packed = gate(qlab_packed, what, "qlab_packed", _I64, dev, (q.shape[0], None))
    dblab_packed = gate(dblab_packed, what, "dblab_packed", _I64, dev, (db.shape[0], None))
    if dblab_packed.shape[1] != qlab_packed.shape[1]:
        raise ValueError(f"{what}: label widths differ")
    return q, db, qlab_packed, dblab_packed, qlab_packed.shape[1], int(k)


def ip_map_at_k(q, db, qlab_packed, dblab_packed, k):
    """mAP@k ingredients of REAL-VALUED embeddings in one launch (wv_ip_map_at_k): rows of `db` ranked by descending inner
    product with each row of `q` (ties: ascending row), AP over the first k -> (ap float32 [Q], nrel int32 [Q]): the numbers,
    bit for bit, map_at_k returns for the lists knn_float(IP, k) makes.  None when the shape is outside the kernel (more
    than IP_MAP_ROWS_MAX rows, D > 512, labels wider than 2 words): the caller then runs those two.
    q [Q, D], db [N, D]: fp32 (bf16 / fp16 are widened); qlab_packed int64 [Q, words], dblab_packed int64 [N, words]."""
    lib = _lib.require_gpu()
    q, db, qlab_packed, dblab_packed, lw, k = _ip_map_args("ip_map_at_k", q, db, qlab_packed, dblab_packed, k, _DEVICE_TYPE)
    if lw > 2:
        return None
    Q = q.shape[0]
    ap, nrel = _ap_buffers(Q, (), q.device)
    if not Q:
        return ap, nrel
    with torch.cuda.device(q.device):
        rc = lib.wv_ip_map_at_k(_lib.ptr(q), _lib.ptr(db), Q, db.shape[0], q.shape[1], _lib.ptr(qlab_packed), _lib.ptr(dblab_packed),
                                lw, k, _lib.ptr(ap), _lib.ptr(nrel), _lib.stream_ptr())
        if rc == _lib.WV_ENOTSUP:
            return None
        _lib.check(rc, "wv_ip_map_at_k")
    return ap, nrel


def hamming_radius_hist(q_packed, db, labels, qlab_packed, nbits):
    """Cumulative distance histograms of every query over ALL rows of `db` and over the rows that share a label with it
    -> (cum, cumrel) int32 [Q, nbits + 2]: cum[q, b] = rows with distance < b (hamming_hist's numbers), cumrel[q, b] = those
    of them relevant to query q.  What precision / recall by Hamming radius need (engine/radius_metrics.py); no [Q, N]
    matrix and no list exists.  The tables add across row shards: more than 32,768 rows (virtual shards) are the sum of the
    per-part calls.  None where hamming_map_at_k answers None (labels wider than 2 words, nbits > 128).
    db: PreparedDB; labels: PreparedLabels of the same rows; qlab_packed: int64 [Q, 1 or 2]."""
    lib = _lib.require_gpu()
    ok, q_packed, qlab_packed = _fused_gate("hamming_radius_hist", q_packed, db, labels, qlab_packed, nbits, code_width=True)
    if not ok:
        return None
    Q = q_packed.shape[0]
    dev = q_packed.device
    if db.parts or labels.parts:
        if not (db.parts and labels.parts) or len(db.parts) != len(labels.parts):
            return None
        cum = torch.zeros((Q, nbits + 2), dtype=torch.int32, device=dev)
        cumrel = torch.zeros_like(cum)
        for part, lab in zip(db.parts, labels.parts):
            got = hamming_radius_hist(q_packed, part, lab, qlab_packed, nbits)
            if got is None:
                return None
            cum += got[0]
            cumrel += got[1]
        return cum, cumrel
    cum = torch.empty((Q, nbits + 2), dtype=torch.int32, device=dev)
    cumrel = torch.empty_like(cum)
    if Q:
        with torch.cuda.device(dev):
            rc = lib.wv_hamming_radius_hist(_lib.ptr(q_packed), _lib.ptr(db.blob), _lib.ptr(labels.blob),
                                            _lib.ptr(qlab_packed), labels.words, Q, db.N, nbits, _lib.ptr(cum),
                                            _lib.ptr(cumrel), _lib.stream_ptr())
            if rc == _lib.WV_ENOTSUP:
                return None
            _lib.check(rc, "wv_hamming_radius_hist")
    return cum, cumrel


def _cutoffs(ks, what):
    """The cut-offs of a multi-k call, as they arrive (any order, repeats allowed) -> (sorted unique list, C int array of
    it, column of every requested cut-off in the sorted list)."""
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError(f"{what}: no cut-offs")
    uniq = sorted(set(ks))
    if len(uniq) > MAX_CUTOFFS:
        raise ValueError(f"{what}: {len(uniq)} different cut-offs (at most {MAX_CUTOFFS} per call)")
    if uniq[0] < 1:
        raise ValueError(f"{what}: cut-off {uniq[0]} must be >= 1")
    return uniq, (ctypes.c_int * len(uniq))(*uniq), [uniq.index(k) for k in ks]


def _columns(ap, nrel, cols):
    """[Q, unique cut-offs] -> [Q, requested cut-offs]; cols None: a single-k call's [Q], as they are"""
    if cols is None or cols == list(range(ap.shape[1])):
        return ap, nrel
    sel = torch.tensor(cols, dtype=torch.long, device=ap.device)
    return ap.index_select(1, sel), nrel.index_select(1, sel)


def _graded_words(lw, what):
    if lw not in (1, 2):
        raise ValueError(f"{what}: {lw} label words (graded overlap takes 1 or 2: up to 128 classes)")
    return lw


def label_overlap_hist(qlab_packed, dblab_packed):
    """hist int32 [Q, 64 * lwords + 1]: hist[q, r] = database rows that share exactly r classes with query q
    (wv_label_overlap_hist: one pass over the packed label words, any N; the tables of row shards add up)."""
    lib = _lib.require_gpu()
    dev = anchor(qlab_packed, "label_overlap_hist", "qlab_packed", _DEVICE_TYPE)
    qlab_packed, dblab_packed, lw = _label_args("label_overlap_hist", qlab_packed, dblab_packed, None, dev)
    _graded_words(lw, "label_overlap_hist")
    Q, N = qlab_packed.shape[0], dblab_packed.shape[0]
    hist = torch.zeros((Q, 64 * lw + 1), dtype=torch.int32, device=qlab_packed.device)
    if Q and N:                                      # an empty shard contributes zeros
        with torch.cuda.device(qlab_packed.device):
            _lib.check(lib.wv_label_overlap_hist(_lib.ptr(qlab_packed), _lib.ptr(dblab_packed), lw, Q, N,
                                                 _lib.ptr(hist), _lib.stream_ptr()), "wv_label_overlap_hist")
    return hist


_NDCG_WEIGHTS = {}               # (device, entries) -> fp64 table w[p] = 1 / log2(p + 2), made on the host by the library


def ndcg_weights(k, device=None):
    """The discount table of wv_ndcg_at_ks, >= k entries (float64), made once per (device, rounded-up length) and kept."""
    n = max(1024, 1 << (int(k) - 1).bit_length())
    key = (str(device) if device is not None else "cpu", n)
    if key not in _NDCG_WEIGHTS:
        w = torch.empty(n, dtype=torch.float64)
        _lib.check(_lib.load().wv_ndcg_weights(_lib.ptr(w), n), "wv_ndcg_weights")
        _NDCG_WEIGHTS[key] = w if device is None else w.to(device)
    return _NDCG_WEIGHTS[key]


def ndcg_at_ks(idx, qlab_packed, dblab_packed, ks, hist=None):
    """DCG and ideal DCG of ranked lists at several cut-offs from one walk (wv_ndcg_at_ks)
    -> (dcg, idcg) float64 [Q, len(ks)].  idx: int32 [Q, >= max(ks)] (int64 is converted); hist: label_overlap_hist of the WHOLE database (made
    here when None).  Gains are 2^overlap - 1 in fp64 (beyond an overlap of 62 the reference's int64 overflows: no parity)."""
    lib = _lib.require_gpu()
    idx, qlab_packed, dblab_packed, lw = _list_args("ndcg_at_ks", idx, qlab_packed, dblab_packed, PITCH)
    _graded_words(lw, "ndcg_at_ks")
    Q, kfull = idx.shape
    uniq, c_ks, cols = _cutoffs(ks, "ndcg_at_ks")
    if uniq[-1] > kfull:
        raise ValueError(f"ndcg_at_ks: cut-off {uniq[-1]} outside the lists' length {kfull}")
    dev = idx.device
    if hist is None:
        hist = label_overlap_hist(qlab_packed, dblab_packed)
    hist = gate(hist, "ndcg_at_ks", "hist (the int32 [Q, 64 * lwords + 1] table of label_overlap_hist)", _I32, dev, (Q, 64 * lw + 1))
    w = ndcg_weights(uniq[-1], dev)
    dcg = torch.zeros((Q, len(uniq)), dtype=torch.float64, device=dev)
    idcg = torch.zeros_like(dcg)
    if Q:
        with torch.cuda.device(dev):
            _lib.check(lib.wv_ndcg_at_ks(_lib.ptr(idx), idx.stride(0), Q, c_ks, len(uniq), _lib.ptr(qlab_packed),
                                         _lib.ptr(dblab_packed), lw, _lib.ptr(hist), _lib.ptr(w),
                                         _lib.ptr(dcg), _lib.ptr(idcg), _lib.stream_ptr()), "wv_ndcg_at_ks")
    return _columns(dcg, idcg, cols)


def _hist_words(nbits):
    """int64 words at the head of a wire row that hold the histogram (nbits + 2 int32, padded to 8 bytes)"""
    return (nbits + 3) // 2


def relbits_wire_words(kin, nbits):
    """int64 words per (query, shard) row of the sharded-mAP wire buffer: [histogram: nbits + 2 int32, padded to 8 bytes |
    relevance string: ceil(kin / 64) uint64]."""
    return _hist_words(nbits) + (kin + 63) // 64


def _wire_args(wire, nbits):
    """The four C arguments that describe a contiguous wire buffer [.., relbits_wire_words]: relevance strings (pointer, row
    pitch in 64-bit words), histograms (pointer, row pitch in int32).  `wire` is a gate() result: its data_ptr() is taken here."""
    ld = wire.shape[-1]
    return wire.data_ptr() + 8 * _hist_words(nbits), ld, wire.data_ptr(), 2 * ld


def hamming_shard_relbits(q_packed, db, labels, qlab_packed, nbits, k, wire=None, kin=None):
    """What a shard contributes to the sharded mAP: per query the relevance string of its k nearest rows (bit p = the p-th
    nearest row shares a label with the query) and its cumulative distance histogram, side by side in ONE int64 buffer
    [Q, relbits_wire_words(kin, nbits)] (kin >= k: the prefix length the ranks agreed on; a shard with fewer rows leaves the
    tail of the string zero) -- a single all_to_all moves both.  `wire`: preallocated (zeroed) buffer.
    -> wire, or None when the shape is outside the fused kernel."""
    lib = _lib.require_gpu()
    ok, q_packed, qlab_packed = _fused_gate("hamming_shard_relbits", q_packed, db, labels, qlab_packed, nbits)
    Q = q_packed.shape[0]
    kin = k if kin is None else kin
    ld = relbits_wire_words(kin, nbits)
    if wire is not None:
        wire = gate(wire, "hamming_shard_relbits", "wire", _I64, q_packed.device, (Q, ld), WRITTEN)
    if not ok or not 1 <= k <= db.N:
        return None
    if wire is None:
        wire = torch.zeros((Q, ld), dtype=torch.int64, device=q_packed.device)
    if Q:
        with torch.cuda.device(q_packed.device):
            rc = lib.wv_hamming_shard_relbits(_lib.ptr(q_packed), _lib.ptr(db.blob), _lib.ptr(labels.blob),
                                              _lib.ptr(qlab_packed), labels.words, *_wire_args(wire, nbits),
                                              Q, db.N, nbits, k, _lib.stream_ptr())
            if rc == _lib.WV_ENOTSUP:
                return None
            _lib.check(rc, "wv_hamming_shard_relbits")
    return wire


def _merge_relbits(what, wire, kin, k, ks, nbits, need_out):
    lib = _lib.require_gpu()
    dev = anchor(wire, what, "wire", _DEVICE_TYPE)
    wire = gate(wire, what, "wire (int64 [G, Q, relbits_wire_words(kin, nbits)])", _I64, dev, (None, None, relbits_wire_words(kin, nbits)))
    G, Q, ld = wire.shape
    if need_out is not None:
        need_out = gate(need_out, what, "need_out", _I32, dev, (1,), WRITTEN)
    cargs, tail, cols, _ = _cuts(what, k, ks)
    ap, nrel = _ap_buffers(Q, tail, wire.device)
    if Q:
        with torch.cuda.device(wire.device):
            rc = getattr(lib, "wv_" + what)(*_wire_args(wire, nbits), G, Q, kin, *cargs, nbits, _lib.ptr(ap), _lib.ptr(nrel),
                                            _lib.ptr(need_out), _lib.stream_ptr())
            if rc == _lib.WV_ENOTSUP:                            # the merged string does not fit the kernel's LDS
                return None
            _lib.check(rc, "wv_" + what)
    return _columns(ap, nrel, cols)


def merge_relbits_map(wire, kin, k, nbits, need_out=None):
    """wire int64 [G, Q, relbits_wire_words(kin, nbits)] -- the rows hamming_shard_relbits made on G contiguous row shards in
    rank order -> (ap float32 [Q], nrel int32 [Q]) of the merged top-k lists, equal to map_at_k of the merged lists, or
    None when the k-bit merged string does not fit the kernel's LDS.  need_out as in topk_merge_cum."""
    return _merge_relbits("merge_relbits_map", wire, kin, k, None, nbits, need_out)


MERGE_LDS_LIMIT = 60 * 1024  # WV_MERGE_RELBITS_LDS_LIMIT: dynamic LDS above which wv_merge_relbits_map[_ks] answer WV_ENOTSUP


def merge_relbits_lds_bytes(G, k, nbits):
    """LDS wv_merge_relbits_map[_ks] need for G shards and a (largest) cut-off k, as the library itself computes it
    (wv_merge_relbits_map_ks_lds_bytes; no GPU needed).  Callers that must decide a fallback before any rank exchanges
    anything (parallel.sharded_hamming_map_at_k) hold it against MERGE_LDS_LIMIT."""
    return int(_lib.load().wv_merge_relbits_map_ks_lds_bytes(int(G), int(k), int(nbits)))


def merge_relbits_map_ks(wire, kin, ks, nbits, need_out=None):
    """merge_relbits_map for several cut-offs from ONE merged string (assembled for max(ks); need_out refers to max(ks))
    -> (ap float32 [Q, len(ks)], nrel int32 [Q, len(ks)]), or None when that string does not fit the kernel's LDS."""
    return _merge_relbits("merge_relbits_map_ks", wire, kin, None, ks, nbits, need_out)


def wire_histograms(wire, nbits):
    """int32 [.., nbits + 2] view of the histograms inside a wire buffer (tests, diagnostics)."""
    return wire.view(torch.int32)[..., :nbits + 2]         # the first 2 * _hist_words(nbits) int32 of a row hold them


def hit_prefix(idx, qlab_packed, dblab_packed):
    """hits[q, p] = number of relevant entries among idx[q, :p+1] (uint32 counts as int32 tensor [Q, k]).
    idx: int32 [Q, k] (int64 is converted); qlab_packed: int64 [Q, words].  As in map_at_k, the values of idx are not checked
    against the rows of dblab_packed (no N in the entry point; a check would cost a reduction and a host read)."""
    lib = _lib.require_gpu()
    idx, qlab_packed, dblab_packed, lw = _list_args("hit_prefix", idx, qlab_packed, dblab_packed, ROWS)
    Q, k = idx.shape
    hits = torch.empty((Q, k), dtype=torch.int32, device=idx.device)
    if Q:
        with torch.cuda.device(idx.device):
            rc = lib.wv_hit_prefix(_lib.ptr(idx), Q, k, _lib.ptr(qlab_packed), _lib.ptr(dblab_packed),
                                   lw, _lib.ptr(hits), _lib.stream_ptr())
            _lib.check(rc, "wv_hit_prefix")
    return hits
