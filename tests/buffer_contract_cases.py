"""The buffer contract of the retrieval and loss entry points as ONE table (ROWS), and the harness that runs a row.
Shared by tests/test_buffer_contract_host.py (host twins, no GPU) and tests/test_gpu_buffer_contract.py.  No test functions.

A Row names an entry point of include/wvhash.h, how to call it through ctypes, its inputs, its outputs (dtype, shape, row
pitch, whether NULL is allowed), its workspace-size function, the blobs that are prepared into guarded memory first, and how
the expected bits are obtained.  Expected values come from the host twins (csrc/host_*.cpp, held bit-equal to the kernels
by the existing tests) and from plain torch on their results -- never from a second GPU call:
  lists, distance rows  wv_hamming_topk_cpu          cum[q][b]     counts of wv_hamming_dist_cpu's matrix below b
  rows16                the twin's list as uint16    relbits       the twin's list pushed through the label words
  merged lists          the twin's unsharded list    ap / nrel     wv_map_at_k_cpu on the twin's list
  hits, hist, dcg/idcg  wv_hit_prefix_cpu, wv_label_overlap_hist_cpu, wv_ndcg_at_ks_cpu
  radius tables         wv_hamming_radius_hist_cpu   losses        wv_pair_loss_cpu / wv_rank_ap_cpu (within TOL, see `check`)
  wv_ip_map_at_k_cpu, wv_group_layernorm_cpu
`oracle` (where a row has a host twin) is the independent expectation the twin itself is held to under the same harness:
oracle/ranking.py, the float64 restatements of the case modules, plain torch.

run_row() places every input, output, blob and workspace through guarded.Guards, calls, and checks rc, guards, pitch gaps
and that no input changed.  Placements: offset 0 (256-byte aligned) or `natural` = one element past it (see NATURAL).

The kernel a shape runs is restated here from csrc/rank.hpp (rank_plan_of) so that the host test can assert that every
listed N / k reaches the RankPlan it is listed for.
"""
import collections
import ctypes
import functools

import numpy as np
import torch

import group_layernorm_cases as GC
import ip_map_cases as IC
import ndcg_cases as NC_
import pair_loss_cases as PC
import radius_cases as RC
import rank_ap_cases as AC
from guarded import Guards, bits
from oracle import ranking
from ranking_cases import spread_codes
from wvhash import _lib, synth
from wvhash.engine import hamming_host as HH

I32, I16, U8, I64, F32, F64, BF16 = torch.int32, torch.int16, torch.uint8, torch.int64, torch.float32, torch.float64, torch.bfloat16
AP_TOL_ORACLE = 1e-6        # test_gpu_ranking.py: AP against the oracle (fp32 quotients, fp64 sums)
AP_TOL_ONE_WAVE = 1.2e-7    # test_fused_map_at_k_equals_ranking_then_ap: one wave per query sums in its own order

# ------------------------------------------------------------------------------------------ csrc/rank.hpp, restated
K_WIN_ROWS, K_MAX_BINS, K_WIN_BINS, RANK_LDS_LIMIT = 33, 130, 32, 100 * 1024
IMG64_MAX_ROWS, IMG256_MAX_ROWS = 64 * 64, 256 * 128


def window_lds_bytes_per_query(tpq, k, bm_words=0):
    b = K_WIN_ROWS * (tpq // 2) * 4
    b += ((k + tpq) * 2 + 15) // 16 * 16
    b += (K_MAX_BINS + 1 + K_WIN_BINS + 4 + 3) // 4 * 4 * 4
    b += bm_words * 4
    b = (b + 15) // 16 * 16
    hist = (K_MAX_BINS + 1) * 17 * 4
    return b if b > hist else (hist + 15) // 16 * 16


def rank_window_kernel(Q, N, k, pin):
    if pin == "0":
        return None
    if N >= 65536 or 2 * (k + 128) >= 65536:
        return None
    fits256 = N <= IMG256_MAX_ROWS and window_lds_bytes_per_query(256, k) <= RANK_LDS_LIMIT
    fits64 = N <= IMG64_MAX_ROWS and 4 * window_lds_bytes_per_query(64, k) <= RANK_LDS_LIMIT
    if pin == "64" and fits64:
        return "window64"
    if pin == "256" and fits256:
        return "window256"
    if fits64 and Q >= 4096:
        return "window64"
    return "window256" if fits256 else ("window64" if fits64 else None)


Plan = collections.namedtuple("Plan", "kernel C NC u16")


def rank_plan_of(Q, N, nbits, k, mode="lists", pin=None):
    """(kernel, items per thread C, distance-cache words NC, column kernel's 16-bit counters) of rank_plan()"""
    kern = rank_window_kernel(Q, N, max(k, 1), pin)
    if kern is None:
        return Plan("column", -(-N // 256), 0, N < 65536) if mode == "lists" else Plan(None, 0, 0, False)
    if mode in ("ap", "relbits") and kern == "window64" and k > 32 * 64:
        kern = "window256"
    if mode == "radius":
        kern = "window256"
    tpq = 64 if kern == "window64" else 256
    C = -(-N // tpq)
    NC = 4 if C <= 16 else 8 if C <= 32 else 16 if C <= 64 else 25 if C <= 100 else 32
    return Plan(kern, C, NC, False)


# ------------------------------------------------------------------------------------------ the table's vocabulary
class Out:
    """One output buffer.  ld: row pitch in elements (2-D outputs; gaps are guarded).  nullable: the header allows NULL.
    inout: the caller zeroes it (need_out), whatever the fill.  check: 'bits' | 'ap' (AP_TOL_ONE_WAVE) | 'loss' (C.check)."""

    def __init__(self, name, dtype, shape, nullable=False, ld=None, inout=False, check="bits"):
        self.name, self.dtype, self.shape, self.nullable, self.ld, self.inout, self.check = name, dtype, tuple(shape), nullable, ld, inout, check


class Blob:
    """A prepared blob: `nbytes(lib)` bytes of guarded memory, filled by `prepare(lib, a, ptr, nbytes)` -> rc before the call"""

    def __init__(self, name, nbytes, prepare):
        self.name, self.nbytes, self.prepare = name, nbytes, prepare


class Row:
    def __init__(self, id, entry, inputs, outs, call, expected, pin=None, blobs=(), workspace=None, twin=None, twin_outs=(),
                 oracle=None, moved=None, plan=None, loss_check=None):
        self.id, self.entry, self.inputs, self.outs, self.call, self.expected = id, entry, inputs, outs, call, expected
        self.pin, self.blobs, self.workspace = pin, blobs, workspace
        self.twin, self.twin_outs, self.oracle = twin, twin_outs, oracle
        self.moved = moved or {}            # input name -> byte offset of the natural placement (alignment picks a path)
        self.plan = plan                    # (Q, N, nbits, k, mode, the Plan it is listed for) or None
        self.loss_check = loss_check        # 'loss' outputs: f(results, expected, what)

    def __repr__(self):
        return self.id


class Args:
    """What a row's call sees: pointers by name (NULL for an absent one), the workspace and the stream"""

    def __init__(self, lib, tensors, ws, stream):
        self.lib, self.t, self.ws, self.stream = lib, tensors, ws, stream
        self.ws_bytes = ctypes.c_size_t(ws.numel() if ws is not None else 0)

    def p(self, name, byte_offset=0):
        t = self.t.get(name)
        return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else ctypes.c_void_p(0)

    @property
    def wsp(self):
        return _lib.ptr(self.ws)


NATURAL = "one element past a 256-byte boundary: dist rows at 1 mod 16, int32 lists at 4, uint16 rows at 2 mod 4, fp64 at 8"


def run_row(row, lib, device, fill, natural=False, null=(), host=False):
    """One guarded call of the row (host: its twin on host memory) -> {output name: host copy}.  Asserts rc == 0, every guard
    and pitch gap intact, every input unchanged."""
    dev = torch.device(device)
    G = Guards(dev)
    src = row.inputs()
    tensors = {}
    for name, t in src.items():
        tensors[name] = G.place_like(t.to(dev), offset=row.moved.get(name, 0) if natural else 0, name=f"{row.id}:{name} (input)")
    outs = [o for o in row.outs if o.name not in null and (not host or o.name in row.twin_outs)]
    for o in outs:
        off = torch.empty((), dtype=o.dtype).element_size() if natural else 0
        f = 0x00 if o.inout else fill
        if o.ld is not None:
            tensors[o.name] = G.pitched(o.shape[0], o.shape[1], o.ld, o.dtype, offset=off, fill=f, name=f"{row.id}:{o.name}")
        else:
            tensors[o.name] = G.place(o.shape, o.dtype, offset=off, fill=f, name=f"{row.id}:{o.name}")
    stream = None if host else _lib.stream_ptr()
    ws = None
    if not host:
        if row.workspace is not None:
            ws = G.place(max(int(row.workspace(lib)), 1), U8, fill=fill, name=f"{row.id}:workspace")[:int(row.workspace(lib))]
        a = Args(lib, tensors, ws, stream)
        for b in row.blobs:
            n = int(b.nbytes(lib))
            assert n > 0, (row.id, b.name)
            tensors[b.name] = G.place(n, U8, fill=fill, name=f"{row.id}:{b.name} (blob)")
            rc = b.prepare(lib, a, _lib.ptr(tensors[b.name]), ctypes.c_size_t(n))
            assert rc == 0, (row.id, b.name, rc, lib.wv_last_error())
    a = Args(lib, tensors, ws, stream)
    rc = (row.twin if host else row.call)(lib, a)
    if not host:
        torch.cuda.synchronize()
    assert rc == 0, (row.id, rc, lib.wv_last_error())
    G.assert_intact()
    for name, t in src.items():
        assert torch.equal(bits(tensors[name].cpu()), bits(t)), f"{row.id}: input {name} changed"
    return {o.name: tensors[o.name].cpu().contiguous() for o in outs}


WV_EINVAL = -22


def run_refused(row, lib, device):
    """The row's call with its workspace and prepared blobs 8 bytes past a 16-byte boundary (include/wvhash.h: opaque buffers
    are 16-byte aligned): the preparation and the call answer WV_EINVAL on the host before any launch -- no pointer is
    read, so this runs on host memory too -- and every buffer keeps its bytes."""
    dev = torch.device(device)
    G = Guards(dev)
    src = row.inputs()
    tensors = {name: G.place_like(t.to(dev), name=f"{row.id}:{name} (input)") for name, t in src.items()}
    written = {}
    for o in row.outs:
        if o.ld is not None:
            written[o.name] = G.pitched(o.shape[0], o.shape[1], o.ld, o.dtype, fill=0xFF, name=f"{row.id}:{o.name}")
        else:
            written[o.name] = G.place(o.shape, o.dtype, fill=0xFF, name=f"{row.id}:{o.name}")
    tensors.update(written)
    stream = _lib.stream_ptr() if dev.type == "cuda" else None
    ws = None
    if row.workspace is not None:
        ws = written["workspace"] = G.place(int(row.workspace(lib)), U8, offset=8, fill=0xFF, name=f"{row.id}:workspace")
    a = Args(lib, tensors, ws, stream)
    for b in row.blobs:
        n = int(b.nbytes(lib))
        tensors[b.name] = written[b.name] = G.place(n, U8, offset=8, fill=0xFF, name=f"{row.id}:{b.name} (blob)")
        rc = b.prepare(lib, a, _lib.ptr(tensors[b.name]), ctypes.c_size_t(n))
        assert rc == WV_EINVAL and b"16-byte aligned" in lib.wv_last_error(), (row.id, b.name, rc, lib.wv_last_error())
    rc = row.call(lib, a)
    assert rc == WV_EINVAL and b"16-byte aligned" in lib.wv_last_error(), (row.id, rc, lib.wv_last_error())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    G.assert_intact()
    for name, t in written.items():
        assert bool((bits(t.cpu()) == 0xFF).all()), f"{row.id}: {name} was written by a refused call"
    for name, t in src.items():
        assert torch.equal(bits(tensors[name].cpu()), bits(t)), f"{row.id}: input {name} changed"


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ Hamming ranking data
LABEL_CLASSES = {64: 38, 128: 80}      # nbits -> classes: one label word with 64-bit codes, two with 128-bit codes


def _i16(idx):
    """int32 row numbers < 65536 -> their uint16 bits in int16 storage"""
    return (idx.int() & 0xffff).to(torch.int32).numpy().astype(np.uint16).view(np.int16).copy()


@functools.lru_cache(maxsize=None)
def rank_data(Q, N, nbits):
    q, r = spread_codes(Q, N, nbits, seed=N + nbits)
    lc = LABEL_CLASSES[nbits]
    ql, rl = synth.multi_hot_labels(Q, lc, 0.10, 1), synth.multi_hot_labels(N, lc, 0.10, 2)
    return dict(q=q, r=r, ql=ql, rl=rl, qp=HH.pack_codes(q), rp=HH.pack_codes(r), qlp=HH.pack_labels(ql), rlp=HH.pack_labels(rl),
                lw=(lc + 63) // 64)


@functools.lru_cache(maxsize=None)
def twin_lists(Q, N, nbits, k, lo=0, hi=None, idx_offset=0):
    d = rank_data(Q, N, nbits)
    return HH.hamming_topk(d["qp"], d["rp"][lo:hi].contiguous(), nbits, k, idx_offset=idx_offset)


@functools.lru_cache(maxsize=None)
def twin_cum(Q, N, nbits, lo=0, hi=None):
    d = rank_data(Q, N, nbits)
    dm = HH.hamming_dist(d["qp"], d["rp"][lo:hi].contiguous(), nbits).long()
    return torch.stack([(dm < b).sum(1) for b in range(nbits + 2)], dim=1).int()


def relevance(idx, qlp, rlp):
    """[Q, k] bool: list entry shares a label bit with the query (entries < 0: not relevant)"""
    rows = rlp[idx.long().clamp(min=0)]                       # [Q, k, lw]
    return ((rows & qlp[:, None, :]) != 0).any(2) & (idx >= 0)


def relbits_of(rel):
    """[Q, k] bool -> int64 [Q, ceil(k / 64)]: bit p % 64 of word p / 64 = rel[:, p]"""
    Q, k = rel.shape
    words = (k + 63) // 64
    b = torch.zeros((Q, words * 64), dtype=torch.int64)
    b[:, :k] = rel.long()
    return (b.view(Q, words, 64) << torch.arange(64, dtype=torch.int64)).sum(2)


@functools.lru_cache(maxsize=None)
def twin_ap(Q, N, nbits, k):
    d = rank_data(Q, N, nbits)
    return HH.map_at_k(twin_lists(Q, N, nbits, k)[0], d["qlp"], d["rlp"])


def oracle_lists(Q, N, nbits, k):
    d = rank_data(Q, N, nbits)
    i, dd = ranking.hamming_topk_stable(d["q"], d["r"], k)
    return i.int(), dd.to(U8)


def oracle_ap(idx, ql, rl):
    """float64 AP and hit count of ranked lists from the +-0/1 label matrices: the definition, fp64 throughout"""
    k = idx.shape[1]
    rel = ((rl[idx.long()] * ql[:, None, :]).sum(2) > 0).double()
    hits = rel.cumsum(1)
    n = rel.sum(1)
    ap = (rel * hits / torch.arange(1, k + 1).double()).sum(1) / n.clamp(min=1)
    return torch.where(n > 0, ap, torch.zeros_like(ap)), n.int()


def _prep_db(Q, N, nbits):
    words = (nbits + 63) // 64
    return Blob("prepared", lambda lib: lib.wv_db_prepared_bytes(N, words),
                lambda lib, a, p, n: lib.wv_db_prepare(a.p("db"), N, words, p, n, a.stream))


def _prep_labels(N, lw):
    return Blob("prepared_labels", lambda lib: lib.wv_rank_labels_prepared_bytes(N, lw),
                lambda lib, a, p, n: lib.wv_rank_labels_prepare(a.p("dblab"), N, lw, p, n, a.stream))


def _ws_topk(Q, N, nbits, k):
    return lambda lib: lib.wv_hamming_topk_workspace_bytes(Q, N, (nbits + 63) // 64, max(k, 1))


def _plan(Q, N, nbits, k, mode, pin):
    return (Q, N, nbits, k, mode, pin, rank_plan_of(Q, N, nbits, k, mode, pin))


def _twin_topk(Q, N, nbits, k, off):
    return lambda lib, a: lib.wv_hamming_topk_cpu(a.p("q"), a.p("db"), a.p("idx"), a.p("dist"), Q, N, nbits, k, off)


def _oracle_topk(Q, N, nbits, k, off):
    def f():
        i, d = oracle_lists(Q, N, nbits, k)
        return {"idx": i + off, "dist": d}
    return f


def hamming_rows(Q, N, nbits, k, pin, which):
    """The rows of one (shape, pin).  which: names of the entry points to list."""
    d = lambda: rank_data(Q, N, nbits)
    lw = (LABEL_CLASSES[nbits] + 63) // 64
    words = (nbits + 63) // 64
    off = 1000
    tag = f"Q{Q}-N{N}-b{nbits}-k{k}-pin{pin}"
    codes = lambda: {"q": d()["qp"], "db": d()["rp"]}
    labelled = lambda: {"q": d()["qp"], "db": d()["rp"], "qlab": d()["qlp"], "dblab": d()["rlp"]}
    lists = lambda: twin_lists(Q, N, nbits, k, idx_offset=off)
    cum = lambda: twin_cum(Q, N, nbits)
    rows = []
    o_idx, o_dist = Out("idx", I32, (Q, k)), Out("dist", U8, (Q, k), nullable=True)
    o_cum = Out("cum", I32, (Q, nbits + 2))
    exp_lists = lambda lib, fill: {"idx": lists()[0], "dist": lists()[1], "cum": cum()}
    tw = dict(twin=_twin_topk(Q, N, nbits, k, off), twin_outs=("idx", "dist"), oracle=_oracle_topk(Q, N, nbits, k, off))
    if "wv_hamming_topk" in which:
        rows.append(Row(f"wv_hamming_topk-{tag}", "wv_hamming_topk", codes, [o_idx, o_dist],
                        lambda lib, a: lib.wv_hamming_topk(a.p("q"), a.p("db"), a.p("idx"), a.p("dist"), Q, N, nbits, k, off, a.wsp,
                                                           a.ws_bytes, a.stream),
                        exp_lists, pin, workspace=_ws_topk(Q, N, nbits, k), plan=_plan(Q, N, nbits, k, "lists", pin), **tw))
    if "wv_hamming_topk_prepared" in which:
        rows.append(Row(f"wv_hamming_topk_prepared-{tag}", "wv_hamming_topk_prepared", codes, [o_idx, o_dist],
                        lambda lib, a: lib.wv_hamming_topk_prepared(a.p("q"), a.p("prepared"), a.p("idx"), a.p("dist"), Q, N, nbits, k,
                                                                    off, a.stream),
                        exp_lists, pin, blobs=[_prep_db(Q, N, nbits)], plan=_plan(Q, N, nbits, k, "lists", pin), **tw))
    if "wv_hamming_topk_ex" in which:
        rows.append(Row(f"wv_hamming_topk_ex-{tag}", "wv_hamming_topk_ex", codes,
                        [o_idx, o_dist, Out("cum", I32, (Q, nbits + 2), nullable=True)],
                        lambda lib, a: lib.wv_hamming_topk_ex(a.p("q"), a.p("db"), None, a.p("idx"), a.p("dist"), a.p("cum"), Q, N, nbits,
                                                              k, off, a.wsp, a.ws_bytes, a.stream),
                        exp_lists, pin, workspace=_ws_topk(Q, N, nbits, k), plan=_plan(Q, N, nbits, k, "lists", pin), **tw))
    if "wv_hamming_topk_ex+prepared" in which:
        rows.append(Row(f"wv_hamming_topk_ex+prepared-{tag}", "wv_hamming_topk_ex", codes,
                        [o_idx, o_dist, Out("cum", I32, (Q, nbits + 2), nullable=True)],
                        lambda lib, a: lib.wv_hamming_topk_ex(a.p("q"), a.p("db"), a.p("prepared"), a.p("idx"), a.p("dist"), a.p("cum"),
                                                              Q, N, nbits, k, off, None, ctypes.c_size_t(0), a.stream),
                        exp_lists, pin, blobs=[_prep_db(Q, N, nbits)], plan=_plan(Q, N, nbits, k, "lists", pin), **tw))
    if "wv_hamming_hist" in which:
        rows.append(Row(f"wv_hamming_hist-{tag}", "wv_hamming_hist", codes, [o_cum],
                        lambda lib, a: lib.wv_hamming_hist(a.p("q"), a.p("db"), None, a.p("cum"), Q, N, nbits, a.wsp, a.ws_bytes, a.stream),
                        lambda lib, fill: {"cum": cum()}, pin, workspace=_ws_topk(Q, N, nbits, 1), plan=_plan(Q, N, nbits, 0, "hist", pin)))
    o_rows = Out("rows", I16, (Q, k))
    exp_rows = lambda lib, fill: {"rows": torch.from_numpy(_i16(twin_lists(Q, N, nbits, k)[0])), "cum": cum()}
    if "wv_hamming_topk_rows16" in which:
        rows.append(Row(f"wv_hamming_topk_rows16-{tag}", "wv_hamming_topk_rows16", codes, [o_rows],
                        lambda lib, a: lib.wv_hamming_topk_rows16(a.p("q"), a.p("db"), None, a.p("rows"), Q, N, nbits, k, a.wsp, a.ws_bytes,
                                                                  a.stream),
                        exp_rows, pin, workspace=_ws_topk(Q, N, nbits, k), plan=_plan(Q, N, nbits, k, "rows16", pin)))
    if "wv_hamming_shard_prefix" in which:
        rows.append(Row(f"wv_hamming_shard_prefix-{tag}", "wv_hamming_shard_prefix", codes, [o_rows, o_cum],
                        lambda lib, a: lib.wv_hamming_shard_prefix(a.p("q"), None, a.p("prepared"), a.p("rows"), a.p("cum"), Q, N, nbits, k,
                                                                   None, ctypes.c_size_t(0), a.stream),
                        exp_rows, pin, blobs=[_prep_db(Q, N, nbits)], plan=_plan(Q, N, nbits, k, "rows16", pin)))
    both = [_prep_db(Q, N, nbits), _prep_labels(N, lw)]
    if "wv_hamming_map_at_k" in which:
        one_wave = rank_plan_of(Q, N, nbits, k, "ap", pin).kernel == "window64"
        rows.append(Row(f"wv_hamming_map_at_k-{tag}", "wv_hamming_map_at_k", labelled,
                        [Out("ap", F32, (Q,), check="ap" if one_wave else "bits"), Out("nrel", I32, (Q,), nullable=True)],
                        lambda lib, a: lib.wv_hamming_map_at_k(a.p("q"), a.p("prepared"), a.p("prepared_labels"), a.p("qlab"), lw, Q, N,
                                                               nbits, k, a.p("ap"), a.p("nrel"), a.stream),
                        lambda lib, fill: dict(zip(("ap", "nrel"), twin_ap(Q, N, nbits, k))), pin, blobs=both,
                        plan=_plan(Q, N, nbits, k, "ap", pin)))
    if "wv_hamming_shard_relbits" in which:
        rw, hw = (k + 63) // 64, (nbits + 3) // 2

        def exp_rel(lib, fill):
            return {"relbits": relbits_of(relevance(twin_lists(Q, N, nbits, k)[0], d()["qlp"], d()["rlp"])), "cum": cum()}
        rows.append(Row(f"wv_hamming_shard_relbits-tight-{tag}", "wv_hamming_shard_relbits", labelled,
                        [Out("relbits", I64, (Q, rw)), o_cum],
                        lambda lib, a: lib.wv_hamming_shard_relbits(a.p("q"), a.p("prepared"), a.p("prepared_labels"), a.p("qlab"), lw,
                                                                    a.p("relbits"), 0, a.p("cum"), 0, Q, N, nbits, k, a.stream),
                        exp_rel, pin, blobs=both, plan=_plan(Q, N, nbits, k, "relbits", pin)))
        ld = hw + rw + 1      # one wire row: [histogram | relevance string | a word nobody owns]

        def exp_wire(lib, fill):
            w = torch.full((Q, ld * 8), fill, dtype=U8).view(I64)
            w[:, :hw].view(I32)[:, :nbits + 2] = cum()
            w[:, hw:hw + rw] = exp_rel(lib, fill)["relbits"]
            return {"wire": w}
        rows.append(Row(f"wv_hamming_shard_relbits-wire-{tag}", "wv_hamming_shard_relbits", labelled, [Out("wire", I64, (Q, ld))],
                        lambda lib, a: lib.wv_hamming_shard_relbits(a.p("q"), a.p("prepared"), a.p("prepared_labels"), a.p("qlab"), lw,
                                                                    a.p("wire", 8 * hw), ld, a.p("wire"), 2 * ld, Q, N, nbits, k, a.stream),
                        exp_wire, pin, blobs=both, plan=_plan(Q, N, nbits, k, "relbits", pin)))
    if "wv_hamming_radius_hist" in which:
        def exp_radius(lib, fill):
            c, cr = HH.hamming_radius_hist(d()["qp"], d()["rp"], d()["rlp"], d()["qlp"], nbits)
            return {"cum": c, "cumrel": cr}

        def ora_radius():
            c, cr = RC.brute_tables(d()["q"], d()["r"], d()["ql"], d()["rl"])
            return {"cum": c, "cumrel": cr}
        rows.append(Row(f"wv_hamming_radius_hist-{tag}", "wv_hamming_radius_hist", labelled, [o_cum, Out("cumrel", I32, (Q, nbits + 2))],
                        lambda lib, a: lib.wv_hamming_radius_hist(a.p("q"), a.p("prepared"), a.p("prepared_labels"), a.p("qlab"), lw, Q, N,
                                                                  nbits, a.p("cum"), a.p("cumrel"), a.stream),
                        exp_radius, pin, blobs=both, plan=_plan(Q, N, nbits, 0, "radius", pin),
                        twin=lambda lib, a: lib.wv_hamming_radius_hist_cpu(a.p("q"), a.p("db"), a.p("qlab"), a.p("dblab"), lw, Q, N, nbits,
                                                                           a.p("cum"), a.p("cumrel")),
                        twin_outs=("cum", "cumrel"), oracle=ora_radius))
    if "wv_db_prepare" in which:
        # the blob is an output of exactly wv_db_prepared_bytes: judged by what its three readers make of it
        ldm = (N + 15) // 16 * 16
        rows.append(Row(f"wv_db_prepare-{tag}", "wv_db_prepare", codes, [o_idx, Out("dist", U8, (Q, k)), Out("dmat", U8, (Q, N), ld=ldm)],
                        lambda lib, a: (lib.wv_hamming_topk_prepared(a.p("q"), a.p("prepared"), a.p("idx"), a.p("dist"), Q, N, nbits, k, off,
                                                                     a.stream)
                                        or lib.wv_hamming_dist_prepared(a.p("q"), a.p("prepared"), a.p("dmat"), ldm, Q, N, words, a.stream)),
                        lambda lib, fill: {"idx": lists()[0], "dist": lists()[1], "dmat": HH.hamming_dist(d()["qp"], d()["rp"], nbits)},
                        pin, blobs=[_prep_db(Q, N, nbits)], plan=_plan(Q, N, nbits, k, "lists", pin), moved={"db": 8}))
    if "wv_rank_labels_prepare" in which:
        rows.append(Row(f"wv_rank_labels_prepare-{tag}", "wv_rank_labels_prepare", labelled, [o_cum, Out("cumrel", I32, (Q, nbits + 2))],
                        lambda lib, a: lib.wv_hamming_radius_hist(a.p("q"), a.p("prepared"), a.p("prepared_labels"), a.p("qlab"), lw, Q, N,
                                                                  nbits, a.p("cum"), a.p("cumrel"), a.stream),
                        lambda lib, fill: dict(zip(("cum", "cumrel"), HH.hamming_radius_hist(d()["qp"], d()["rp"], d()["rlp"], d()["qlp"], nbits))),
                        pin, blobs=both, plan=_plan(Q, N, nbits, 0, "radius", pin)))
    return rows


def hamming_dist_row(Q, N, nbits):
    """wv_hamming_dist on a plain database: the same tile loads as wv_db_prepare's permutation (csrc/hamming.hip)"""
    d = lambda: rank_data(Q, N, nbits)
    words, ldm = (nbits + 63) // 64, (N + 15) // 16 * 16
    return Row(f"wv_hamming_dist-Q{Q}-N{N}-b{nbits}", "wv_hamming_dist", lambda: {"q": d()["qp"], "db": d()["rp"]},
               [Out("dmat", U8, (Q, N), ld=ldm)],
               lambda lib, a: lib.wv_hamming_dist(a.p("q"), a.p("db"), a.p("dmat"), ldm, Q, N, words, a.stream),
               lambda lib, fill: {"dmat": HH.hamming_dist(d()["qp"], d()["rp"], nbits)},
               twin=lambda lib, a: lib.wv_hamming_dist_cpu(a.p("q"), a.p("db"), a.p("dmat"), ldm, Q, N, words), twin_outs=("dmat",),
               oracle=lambda: {"dmat": ranking.hamming_matrix_u8(d()["q"], d()["r"]).to(U8)}, moved={"db": 8})


def rank_from_dist_row(Q, N, nbits, k, ld):
    d = lambda: rank_data(Q, N, nbits)

    def inputs():
        m = torch.zeros((Q, ld), dtype=U8)                       # gap columns hold distance 0: read, they would lead every list
        m[:, :N] = HH.hamming_dist(d()["qp"], d()["rp"], nbits)
        return {"dmat": m}
    return Row(f"wv_rank_from_dist-Q{Q}-N{N}-b{nbits}-k{k}-ld{ld}", "wv_rank_from_dist", inputs,
               [Out("idx", I32, (Q, k)), Out("dist", U8, (Q, k))],
               lambda lib, a: lib.wv_rank_from_dist(a.p("dmat"), ld, Q, N, nbits, a.p("idx"), a.p("dist"), k, a.stream),
               lambda lib, fill: dict(zip(("idx", "dist"), twin_lists(Q, N, nbits, k))), moved={"dmat": 1})


# ------------------------------------------------------------------------------------------ merges and list consumers
G_SHARDS = 3


def shard_bounds(N, G=G_SHARDS):
    per = -(-N // G)
    return per, [(min(N, g * per), min(N, (g + 1) * per)) for g in range(G)]


@functools.lru_cache(maxsize=None)
def shard_inputs(Q, N, nbits, k):
    """What G ragged shards send for a top-k search: padded int32 / uint8 lists, 16-bit local lists, histograms, relevance strings"""
    d = rank_data(Q, N, nbits)
    per, bounds = shard_bounds(N)
    kin = min(k, per)
    idx = torch.full((G_SHARDS, Q, kin), -1, dtype=I32)
    dist = torch.full((G_SHARDS, Q, kin), nbits + 1, dtype=U8)
    loc = torch.zeros((G_SHARDS, Q, kin), dtype=I16)
    cum = torch.zeros((G_SHARDS, Q, nbits + 2), dtype=I32)
    rel = torch.zeros((G_SHARDS, Q, (kin + 63) // 64), dtype=I64)
    for g, (lo, hi) in enumerate(bounds):
        kk = min(kin, hi - lo)
        i, dd = twin_lists(Q, N, nbits, kk, lo, hi, lo)
        idx[g, :, :kk], dist[g, :, :kk] = i, dd
        loc[g, :, :kk] = torch.from_numpy(_i16(i - lo))
        cum[g] = twin_cum(Q, N, nbits, lo, hi)
        r = torch.zeros((Q, kin), dtype=torch.bool)
        r[:, :kk] = relevance(i, d["qlp"], d["rlp"])
        rel[g] = relbits_of(r)
    tot = cum.sum(0).long()
    T = (tot[:, 1:] >= k).int().argmax(dim=1)
    need = int(torch.gather(cum.long(), 2, (T + 1).view(1, Q, 1).expand(G_SHARDS, Q, 1)).max())
    return dict(idx=idx, dist=dist, loc=loc, cum=cum, rel=rel, kin=kin, per=per, need=need)


def merge_rows(Q, N, nbits, k):
    s = lambda: shard_inputs(Q, N, nbits, k)
    d = lambda: rank_data(Q, N, nbits)
    per, _ = shard_bounds(N)
    kin = min(k, per)
    tag = f"Q{Q}-N{N}-b{nbits}-k{k}-G{G_SHARDS}"
    o = [Out("idx", I32, (Q, k)), Out("dist", U8, (Q, k))]
    exp = lambda lib, fill: dict(zip(("idx", "dist"), twin_lists(Q, N, nbits, k)))
    expn = lambda lib, fill: dict(exp(lib, fill), need=torch.tensor([s()["need"]], dtype=I32))
    compact = lambda: {"loc": s()["loc"], "cum_in": s()["cum"]}
    rw = (kin + 63) // 64
    return [
        Row(f"wv_topk_merge-{tag}", "wv_topk_merge", lambda: {"idx_in": s()["idx"], "dist_in": s()["dist"]}, o,
            lambda lib, a: lib.wv_topk_merge(a.p("idx_in"), a.p("dist_in"), G_SHARDS, Q, kin, a.p("idx"), a.p("dist"), k, nbits, a.stream), exp),
        Row(f"wv_topk_merge_cum-{tag}", "wv_topk_merge_cum", compact, o,
            lambda lib, a: lib.wv_topk_merge_cum(a.p("loc"), a.p("cum_in"), G_SHARDS, Q, kin, per, a.p("idx"), a.p("dist"), k, nbits, a.stream),
            exp),
        Row(f"wv_topk_merge_cum_need-{tag}", "wv_topk_merge_cum_need", compact, o + [Out("need", I32, (1,), inout=True)],
            lambda lib, a: lib.wv_topk_merge_cum_need(a.p("loc"), a.p("cum_in"), G_SHARDS, Q, kin, per, a.p("idx"), a.p("dist"), k, nbits,
                                                      a.p("need"), a.stream), expn),
        Row(f"wv_merge_relbits_map-{tag}", "wv_merge_relbits_map", lambda: {"rel": s()["rel"], "cum_in": s()["cum"]},
            [Out("ap", F32, (Q,)), Out("nrel", I32, (Q,), nullable=True), Out("need", I32, (1,), inout=True)],
            lambda lib, a: lib.wv_merge_relbits_map(a.p("rel"), rw, a.p("cum_in"), nbits + 2, G_SHARDS, Q, kin, k, nbits, a.p("ap"),
                                                    a.p("nrel"), a.p("need"), a.stream),
            lambda lib, fill: dict(zip(("ap", "nrel"), twin_ap(Q, N, nbits, k)), need=torch.tensor([s()["need"]], dtype=I32))),
    ]


def consumer_rows(Q, N, nbits, k):
    d = lambda: rank_data(Q, N, nbits)
    lw = (LABEL_CLASSES[nbits] + 63) // 64
    tag = f"Q{Q}-N{N}-b{nbits}-k{k}"
    lab = lambda: {"qlab": d()["qlp"], "dblab": d()["rlp"]}
    lst = lambda: dict(lab(), idx=twin_lists(Q, N, nbits, k)[0])
    o_ap = [Out("ap", F32, (Q,)), Out("nrel", I32, (Q,), nullable=True)]
    exp_ap = lambda lib, fill: dict(zip(("ap", "nrel"), twin_ap(Q, N, nbits, k)))

    def ora_ap():
        ap, n = oracle_ap(oracle_lists(Q, N, nbits, k)[0], d()["ql"], d()["rl"])
        return {"ap": ap, "nrel": n}
    rows = [Row(f"wv_map_at_k-{tag}", "wv_map_at_k", lst, o_ap,
                lambda lib, a: lib.wv_map_at_k(a.p("idx"), Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("ap"), a.p("nrel"), a.stream), exp_ap,
                twin=lambda lib, a: lib.wv_map_at_k_cpu(a.p("idx"), k, Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("ap"), a.p("nrel")),
                twin_outs=("ap", "nrel"), oracle=ora_ap)]
    for ld in (k, k + 3):
        wide = lambda ld=ld: dict(lab(), idx=twin_lists(Q, N, nbits, ld)[0])      # the list at k = ld: its tail is never to be read
        rows.append(Row(f"wv_map_at_k_ld-{tag}-ld{ld}", "wv_map_at_k_ld", wide, o_ap,
                        lambda lib, a, ld=ld: lib.wv_map_at_k_ld(a.p("idx"), ld, Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("ap"), a.p("nrel"),
                                                                 a.stream), exp_ap,
                        twin=lambda lib, a, ld=ld: lib.wv_map_at_k_cpu(a.p("idx"), ld, Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("ap"),
                                                                       a.p("nrel")),
                        twin_outs=("ap", "nrel"), oracle=ora_ap))
    rows.append(Row(f"wv_hit_prefix-{tag}", "wv_hit_prefix", lst, [Out("hits", I32, (Q, k))],
                    lambda lib, a: lib.wv_hit_prefix(a.p("idx"), Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("hits"), a.stream),
                    lambda lib, fill: {"hits": HH.hit_prefix(twin_lists(Q, N, nbits, k)[0], d()["qlp"], d()["rlp"])},
                    twin=lambda lib, a: lib.wv_hit_prefix_cpu(a.p("idx"), Q, k, a.p("qlab"), a.p("dblab"), lw, a.p("hits")),
                    twin_outs=("hits",),
                    oracle=lambda: {"hits": ((d()["rl"][oracle_lists(Q, N, nbits, k)[0].long()] * d()["ql"][:, None, :]).sum(2) > 0)
                                    .int().cumsum(1).int()}))
    nh = 64 * lw + 1

    def ora_hist():
        ov = torch.from_numpy(NC_.overlaps(d()["ql"].numpy(), d()["rl"].numpy()))
        return {"hist": torch.stack([torch.bincount(ov[i], minlength=nh) for i in range(Q)]).int()}
    rows.append(Row(f"wv_label_overlap_hist-{tag}", "wv_label_overlap_hist", lab, [Out("hist", I32, (Q, nh))],
                    lambda lib, a: lib.wv_label_overlap_hist(a.p("qlab"), a.p("dblab"), lw, Q, N, a.p("hist"), a.stream),
                    lambda lib, fill: {"hist": HH.label_overlap_hist(d()["qlp"], d()["rlp"])},
                    twin=lambda lib, a: lib.wv_label_overlap_hist_cpu(a.p("qlab"), a.p("dblab"), lw, Q, N, a.p("hist")),
                    twin_outs=("hist",), oracle=ora_hist))
    ks = [c for c in (1, 20, 37) if c <= k] or [k]
    c_ks = (ctypes.c_int * len(ks))(*ks)

    def ndcg_in():
        w = torch.empty(max(ks), dtype=F64)
        assert _lib.load().wv_ndcg_weights(_lib.ptr(w), max(ks)) == 0
        return dict(lst(), hist=HH.label_overlap_hist(d()["qlp"], d()["rlp"]), w=w)

    def ora_ndcg():
        rel = NC_.overlaps(d()["ql"].numpy(), d()["rl"].numpy())
        rank = oracle_lists(Q, N, nbits, k)[0].numpy()
        cols = [NC_.dcg_sums(rank, rel, c) for c in ks]
        return {"dcg": torch.from_numpy(np.stack([c[0] for c in cols], 1)), "idcg": torch.from_numpy(np.stack([c[1] for c in cols], 1))}
    rows.append(Row(f"wv_ndcg_at_ks-{tag}", "wv_ndcg_at_ks", ndcg_in, [Out("dcg", F64, (Q, len(ks))), Out("idcg", F64, (Q, len(ks)))],
                    lambda lib, a: lib.wv_ndcg_at_ks(a.p("idx"), k, Q, c_ks, len(ks), a.p("qlab"), a.p("dblab"), lw, a.p("hist"), a.p("w"),
                                                     a.p("dcg"), a.p("idcg"), a.stream),
                    lambda lib, fill: dict(zip(("dcg", "idcg"), HH.ndcg_at_ks(twin_lists(Q, N, nbits, k)[0], d()["qlp"], d()["rlp"], ks))),
                    twin=lambda lib, a: lib.wv_ndcg_at_ks_cpu(a.p("idx"), k, Q, c_ks, len(ks), a.p("qlab"), a.p("dblab"), lw, a.p("hist"),
                                                              a.p("w"), a.p("dcg"), a.p("idcg")),
                    twin_outs=("dcg", "idcg"), oracle=ora_ndcg))
    rows[-1].ks = ks
    return rows


# ------------------------------------------------------------------------------------------ losses and the batch proxy
def pair_loss_row(case):
    x = lambda: PC.inputs(case)
    B, D = case.B, case.D
    lw = (case.C + 63) // 64
    prm = lambda: PC.params_of(x())

    @functools.lru_cache(maxsize=None)
    def twin():
        out, grad = torch.empty(3, dtype=F32), torch.empty((B, D), dtype=F32)
        p = prm()
        assert _lib.load().wv_pair_loss_cpu(_lib.ptr(x().e), _lib.ptr(x().packed), lw, B, D, ctypes.byref(p), _lib.ptr(out), _lib.ptr(grad)) == 0
        return out, grad

    def call(lib, a):
        p = prm()
        return lib.wv_pair_loss(a.p("e"), a.p("labels"), lw, B, D, ctypes.byref(p), a.p("out"), a.p("grad"), a.wsp, a.ws_bytes, a.stream)

    def tw(lib, a):
        p = prm()
        return lib.wv_pair_loss_cpu(a.p("e"), a.p("labels"), lw, B, D, ctypes.byref(p), a.p("out"), a.p("grad"))
    return Row(f"wv_pair_loss-{PC.case_id(case)}", "wv_pair_loss", lambda: {"e": x().e.contiguous(), "labels": x().packed.contiguous()},
               [Out("out", F32, (3,), check="loss"), Out("grad", F32, (B, D), nullable=True, check="loss")], call,
               lambda lib, fill: dict(zip(("out", "grad"), twin())), workspace=lambda lib: lib.wv_pair_loss_workspace_bytes(B, D),
               twin=tw, twin_outs=("out", "grad"), oracle=lambda: dict(zip(("out", "grad"), PC.reference(case))),
               loss_check=lambda got, want, what: PC.check(got["out"], got.get("grad"), want["out"], want["grad"], what))


def rank_ap_row(case):
    x = lambda: AC.inputs(case)
    B, M = case.B, case.M
    prm = lambda: AC.params_of(x())
    form = _lib.WV_RANK_AP_QUICK if case.form == "quick" else _lib.WV_RANK_AP_GENERAL

    @functools.lru_cache(maxsize=None)
    def twin():
        ap, grad = torch.empty(B, dtype=F32), torch.empty((B, M), dtype=F32)
        p = prm()
        assert _lib.load().wv_rank_ap_cpu(_lib.ptr(x().scores), _lib.ptr(x().target), B, M, ctypes.byref(p), _lib.ptr(ap), _lib.ptr(grad)) == 0
        return ap, grad

    def call(lib, a):
        p = prm()
        return lib.wv_rank_ap(a.p("scores"), a.p("target"), B, M, ctypes.byref(p), a.p("ap"), a.p("grad"), a.wsp, a.ws_bytes, a.stream)

    def tw(lib, a):
        p = prm()
        return lib.wv_rank_ap_cpu(a.p("scores"), a.p("target"), B, M, ctypes.byref(p), a.p("ap"), a.p("grad"))
    return Row(f"wv_rank_ap-{AC.case_id(case)}", "wv_rank_ap", lambda: {"scores": x().scores.contiguous(), "target": x().target.contiguous()},
               [Out("ap", F32, (B,), check="loss"), Out("grad", F32, (B, M), nullable=True, check="loss")], call,
               lambda lib, fill: dict(zip(("ap", "grad"), twin())), workspace=lambda lib: lib.wv_rank_ap_workspace_bytes(B, M, form),
               twin=tw, twin_outs=("ap", "grad"), oracle=lambda: dict(zip(("ap", "grad"), AC.reference(case))),
               loss_check=lambda got, want, what: AC.check(got["ap"], got.get("grad"), want["ap"], want["grad"], what))


def ip_map_row(case):
    x = lambda: IC.inputs(case)
    c = case
    call_args = lambda a: (a.p("q"), a.p("db"), c.Q, c.N, c.D, a.p("qlab"), a.p("dblab"), c.lwords, c.k, a.p("ap"), a.p("nrel"))
    return Row(f"wv_ip_map_at_k-{IC.case_id(case)}", "wv_ip_map_at_k",
               lambda: {"q": x().q.contiguous(), "db": x().db.contiguous(), "qlab": x().qlp.contiguous(), "dblab": x().rlp.contiguous()},
               [Out("ap", F32, (c.Q,)), Out("nrel", I32, (c.Q,), nullable=True)],
               lambda lib, a: lib.wv_ip_map_at_k(*call_args(a), a.stream),
               lambda lib, fill: dict(zip(("ap", "nrel"), HH.ip_map_at_k(x().q, x().db, x().qlp, x().rlp, c.k))),
               twin=lambda lib, a: lib.wv_ip_map_at_k_cpu(*call_args(a)), twin_outs=("ap", "nrel"),
               oracle=lambda: dict(zip(("ap", "nrel"), IC.oracle_ap(case))), moved={"db": 4})


def group_layernorm_row(c, x_dtype, out_dtype):
    ins = functools.lru_cache(maxsize=None)(lambda: GC.make_inputs(c, x_dtype))
    N, T, E, G = c["N"], c["T"], c["E"], c["G"]
    args = lambda a: (a.p("x"), GC.DT_CODE[x_dtype], a.p("out"), GC.DT_CODE[out_dtype], N, T, E, G, a.p("gamma"), a.p("beta"),
                      ctypes.c_float(c["eps"]))
    name = {F32: "f32", BF16: "bf16"}
    return Row(f"wv_group_layernorm-{GC.case_id(c)}-{name[x_dtype]}-{name[out_dtype]}", "wv_group_layernorm",
               lambda: dict(zip(("x", "gamma", "beta"), ins())), [Out("out", out_dtype, (N, T, E))],
               lambda lib, a: lib.wv_group_layernorm(*args(a), a.stream),
               lambda lib, fill: {"out": GC.run_twin(*ins(), c["eps"], G, out_dtype)},
               twin=lambda lib, a: lib.wv_group_layernorm_cpu(*args(a)), twin_outs=("out",),
               oracle=lambda: {"out": GC.reference_f64(*ins(), c["eps"], G), "stock": GC.chunk_norm_cat(ins()[0].float(), ins()[1], ins()[2], c["eps"], G)},
               moved={"x": torch.empty((), dtype=x_dtype).element_size()})


# ------------------------------------------------------------------------------------------ the table
RANK_Q, RANK_N = 17, 700
RANK_KS = (1, 37, 700)
PINS = ("0", "64", "256", None)
LIST_ENTRIES = ("wv_hamming_topk", "wv_hamming_topk_prepared", "wv_hamming_topk_ex", "wv_hamming_topk_ex+prepared", "wv_db_prepare")
WINDOW_ENTRIES = ("wv_hamming_hist", "wv_hamming_topk_rows16", "wv_hamming_shard_prefix", "wv_hamming_map_at_k",
                  "wv_hamming_shard_relbits")
RADIUS_ENTRIES = ("wv_hamming_radius_hist", "wv_rank_labels_prepare")
# instantiation edges of the windowed kernel: N -> the (C, NC) it is listed for
EDGES_256 = {4097: (17, 8), 8193: (33, 16), 16385: (65, 25), 25601: (101, 32), 32768: (128, 32)}
EDGES_64 = {1025: (17, 8), 2049: (33, 16), 4096: (64, 16)}
U32_COLUMN = dict(Q=2, N=65539, nbits=64, k=37)


def _rows():
    rows = []
    for nbits in (64, 128):
        for k in RANK_KS:
            for pin in PINS:
                which = LIST_ENTRIES + (WINDOW_ENTRIES if pin != "0" else ()) + (RADIUS_ENTRIES if pin in ("256", None) and k == 37 else ())
                if k != 37:            # the histogram does not depend on k: once per (nbits, pin)
                    which = tuple(w for w in which if w != "wv_hamming_hist")
                rows += hamming_rows(RANK_Q, RANK_N, nbits, k, pin, which)
            for ld in (RANK_N, RANK_N + 3):
                rows.append(rank_from_dist_row(RANK_Q, RANK_N, nbits, k, ld))
        rows.append(hamming_dist_row(RANK_Q, RANK_N, nbits))
        for k in (37, 700):
            rows += merge_rows(RANK_Q, RANK_N, nbits, k)
        rows += consumer_rows(RANK_Q, RANK_N, nbits, 37)
    u = U32_COLUMN
    rows += hamming_rows(u["Q"], u["N"], u["nbits"], u["k"], None, ("wv_hamming_topk_ex",))
    for pin, edges in (("256", EDGES_256), ("64", EDGES_64)):
        for N in edges:
            rows += hamming_rows(3, N, 64, 37, pin, ("wv_hamming_topk_ex",))
    for B, D in ((9, 65), (33, 64), (9, 300)):
        rows += [pair_loss_row(c) for c in PC.CASES if (c.B, c.D) == (B, D) and c.kind in ("sch_tanh", "hashnet_s3")]
    for name, form in (("65x65", "quick"), ("65x65", "general"), ("5x130", "general"), ("257x257", "quick")):
        rows += [rank_ap_row(c) for c in AC.CASES if c.name == name and c.form == form and c.kind == "sup"]
    ragged = [c for c in IC.ALL_CASES if c.kind == "grid" and c.N % 256 != 0 and c.N > 2]
    rows.append(ip_map_row(min((c for c in ragged if c.D % 4 == 0), key=lambda c: (c.N, c.D))))
    rows.append(ip_map_row(min((c for c in ragged if c.D % 4 != 0), key=lambda c: (c.N, c.D))))
    for E in (100, 515):
        c = next(c for c in GC.CASES if c["E"] == E and c["kind"] == "randn")
        rows += [group_layernorm_row(c, xd, od) for xd in GC.DTYPES for od in GC.DTYPES]
    ids = [r.id for r in rows]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    return rows


ROWS = _rows()

# every device entry point the contract covers (the table must have a row for each)
ENTRY_POINTS = ("wv_hamming_dist", "wv_hamming_topk", "wv_hamming_topk_prepared", "wv_hamming_topk_ex", "wv_hamming_hist", "wv_hamming_topk_rows16",
                "wv_hamming_shard_prefix", "wv_hamming_map_at_k", "wv_hamming_shard_relbits", "wv_hamming_radius_hist", "wv_db_prepare",
                "wv_rank_labels_prepare", "wv_rank_from_dist", "wv_topk_merge", "wv_topk_merge_cum", "wv_topk_merge_cum_need",
                "wv_merge_relbits_map", "wv_map_at_k", "wv_map_at_k_ld", "wv_hit_prefix", "wv_label_overlap_hist", "wv_ndcg_at_ks",
                "wv_pair_loss", "wv_rank_ap", "wv_ip_map_at_k", "wv_group_layernorm")
