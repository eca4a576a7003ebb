"""Database-sharded Hamming retrieval across the GPUs of one node (one process per GPU, RCCL).

Reference analogue: faiss.index_cpu_to_all_gpus(index, co) with co.shards = True
(/root/reference/main/engine/get_knn.py:41-44): database rows split across GPUs, brute-force search
per shard, per-shard top-k merged on the HOST.  Here the shards stay resident in HBM as packed codes,
and the only exchange steps are
  1. all_gather of the packed query codes (Q * nbits/8 bytes per rank -- tiny), so every rank can rank
     every query against its shard;
  2. all_to_all of the per-shard list prefixes: rank r receives, from every shard, the lists of ITS queries only
     (an all_gather would move world_size times more) -- as 16-bit local row numbers plus the shard's cumulative
     distance histogram per query (compact form), or int32 index + uint8 distance when a shard has > 65536 rows;
  3. a local G-way merge on the GPU (wv_topk_merge_cum / wv_topk_merge), exact and identical for every world
     size because lists are ordered by (distance, global index) and shards are contiguous row ranges in rank order.
xGMI is point-to-point: with 8 GPUs fully connected both collectives are one direct exchange per peer.
"""
import torch
import torch.distributed as dist

from .engine import hamming as H


def shard_bounds(n_rows, world_size, rank):
    per = (n_rows + world_size - 1) // world_size
    lo = min(n_rows, rank * per)
    hi = min(n_rows, lo + per)
    return lo, hi, per


def _cpu_staged(group):
    """gloo moves host memory only: stage through the CPU (rehearsal path; RCCL takes device tensors)."""
    return dist.get_backend(group) == "gloo"


class ExchangeTrace:
    """What the sharded search puts on the wire: every collective of this module is counted (calls, payload bytes of this
    rank) and, with timing=True, bracketed by HIP events on the calling stream (the collective's own stream is joined to it
    by torch before the call returns, so the pair spans queueing + transfer).  Install with `parallel.TRACE = ExchangeTrace()`;
    bench.py asserts one all_gather + one all_to_all per steady-state step with it and reports per-rank milliseconds."""

    def __init__(self, timing=False):
        self.timing = timing
        self.calls = {"all_gather": 0, "all_to_all": 0, "all_reduce": 0}
        self.bytes = {"all_gather": 0, "all_to_all": 0, "all_reduce": 0}
        self.events = []                                  # (name, start, end)

    def ms(self):
        out = {"all_gather": 0.0, "all_to_all": 0.0, "all_reduce": 0.0}
        for name, e0, e1 in self.events:
            out[name] += e0.elapsed_time(e1)
        return out


TRACE = None


class _traced:
    def __init__(self, name, t):
        self.name, self.t, self.e0 = name, t, None

    def __enter__(self):
        tr = TRACE
        if tr is not None:
            tr.calls[self.name] += 1
            tr.bytes[self.name] += self.t.numel() * self.t.element_size()
            if tr.timing and self.t.is_cuda:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.e0 is not None and TRACE is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            TRACE.events.append((self.name, self.e0, e1))
        return False


def _all_gather(out, inp, group):
    with _traced("all_gather", inp):
        if _cpu_staged(group) and inp.is_cuda:
            o, i = out.cpu(), inp.cpu()
            dist.all_gather_into_tensor(o, i, group=group)
            out.copy_(o)
        else:
            dist.all_gather_into_tensor(out, inp, group=group)


def _all_to_all(out, inp, group):
    with _traced("all_to_all", inp):
        if _cpu_staged(group) and inp.is_cuda:
            o, i = out.cpu(), inp.cpu()
            dist.all_to_all_single(o, i, group=group)
            out.copy_(o)
        else:
            dist.all_to_all_single(out, inp, group=group)


def pad_value(nbits):
    """Distance assigned to padding entries of ragged shard lists: sorts after every real entry."""
    return nbits + 1


def _all_reduce(t, op, group):
    with _traced("all_reduce", t):
        if _cpu_staged(group) and t.is_cuda:
            c = t.cpu()
            dist.all_reduce(c, op=op, group=group)
            t.copy_(c)
        else:
            dist.all_reduce(t, op=op, group=group)


def _gather_rows(local, world, group):
    """all_gather of every rank's [Ql, width] rows -> [world * Ql, width], in rank order"""
    out = torch.empty((world * local.shape[0], local.shape[1]), dtype=local.dtype, device=local.device)
    _all_gather(out, local.contiguous(), group)
    return out


def _prefix_len(kin, hint):
    """The prefix length exchanged for a hint (or a measured need): at least one entry, at most what a shard can owe"""
    return max(1, min(int(kin), int(hint)))


def _exact_send(cum, k, kin, group, send_hint=None):
    """Exact sizing of an exchange from this shard's histograms cum [Q, nbits + 2]: their SUM all-reduce (Q * (nbits + 2) * 4
    bytes) gives every rank the global k-th distance T of every query, H.owed_prefix this shard's longest prefix with
    distance <= T (`need`, device int32 [1]).  Without a hint the prefix length is the maximum over all ranks -- one scalar
    MAX all-reduce and the one host read of the exchange --, so the exchange stays a fixed-size all_to_all.  With a hint every
    rank sends `send_hint` entries and `need` stays THIS shard's own requirement: no MAX all-reduce, no host read; the
    caller verifies need <= send_hint on every rank whenever it synchronises anyway (exchange_ok).  -> (send, need)"""
    cum_g = cum.clone()
    _all_reduce(cum_g, dist.ReduceOp.SUM, group)
    need = H.owed_prefix(cum, cum_g, k)
    if send_hint is None:
        _all_reduce(need, dist.ReduceOp.MAX, group)
        send_hint = need.item()
    return _prefix_len(kin, send_hint), need


def _exchange_compact(rows, cum, send, world, per, k, nbits, group, report_need):
    """Compact exchange and merge: 16-bit LOCAL row numbers (2 bytes per entry) and, instead of a distance row, the shard's
    cumulative histogram of each query (a sorted list is fully described by it): 2 bytes per entry + 4 * (nbits + 2) bytes per
    (query, shard) on the wire instead of 5 bytes per entry.  int16 storage, shipped as bytes (RCCL has no 16-bit integer
    type).  report_need: the merge kernel has every shard's histograms of its queries, derives each query's global k-th
    distance and reports the longest prefix any shard owed.  -> (idx, dist, need int32 [1] or None)"""
    if rows.shape[1] < send:                            # a shard shorter than the prefix: pad (never read by the merge)
        rows = torch.nn.functional.pad(rows, (0, send - rows.shape[1]))
    rows_r = torch.empty_like(rows)
    _all_to_all(rows_r.view(torch.uint8), rows.contiguous().view(torch.uint8), group)
    cum_r = torch.empty_like(cum)
    _all_to_all(cum_r, cum.contiguous(), group)
    need = torch.zeros(1, dtype=torch.int32, device=rows.device) if report_need else None
    Ql = rows.shape[0] // world                         # received layout: [shard g][my Ql queries][...]
    idx, d = H.topk_merge_cum(rows_r.view(world, Ql, send), cum_r.view(world, Ql, nbits + 2), per, k, nbits, need_out=need)
    return idx, d, need


def _exchange_wide(lists, nq, send, world, k, nbits, device, group):
    """Exchange and merge of int32 global rows + uint8 distances: shards of more than 65,536 rows, trim=False.
    lists: (idx, dist) of this shard, or None for an empty one."""
    idx_s = torch.full((nq, send), -1, dtype=torch.int32, device=device)
    dist_s = torch.full((nq, send), pad_value(nbits), dtype=torch.uint8, device=device)
    if lists is not None:
        w = min(send, lists[0].shape[1])
        idx_s[:, :w], dist_s[:, :w] = lists[0][:, :w], lists[1][:, :w]
    idx_r = torch.empty_like(idx_s)                     # block j of my lists (queries of rank j) goes to rank j
    dist_r = torch.empty_like(dist_s)
    _all_to_all(idx_r, idx_s, group)
    _all_to_all(dist_r, dist_s, group)
    Ql = nq // world                                    # received layout: [shard g][my Ql queries][send]
    return H.topk_merge(idx_r.view(world, Ql, send), dist_r.view(world, Ql, send), k, nbits)


def sharded_hamming_topk(q_local, db_shard, nbits, k, n_total, group=None, workspace=None, trim=True,
                         send_hint=None, return_need=False, want_dist=True):
    """q_local: packed codes of THIS rank's queries [Ql, words]; db_shard: this rank's rows
    [lo:hi] of the packed database (tensor or PreparedDB).  Returns the global (idx int32 [Ql,k], dist uint8
    [Ql,k]) of the local queries.  Every rank must call with the same Ql.

    trim=True: the exchange is sized exactly first (_exact_send): a shard only has to send its list prefix with distance
    <= T, the query's global k-th distance -- typically ~k/world + ties entries per query instead of min(k, shard rows).

    send_hint (with trim): prefix length to exchange WITHOUT the host read -- for a steady stream of query batches
    (serving, bench.py) whose needed length is known from earlier batches.  The call then never synchronises with the
    host and runs no all-reduce (one ranking pass per shard, two all_to_alls, the merge); the result is exact iff the
    returned `need` (device int32 [1], return_need=True: the longest prefix any shard owed one of THIS rank's queries) is
    <= send_hint on every rank, which the caller checks whenever it next synchronises anyway (`exchange_ok`).

    want_dist=False: the caller only needs the ranked lists (mAP does: calculate_maphashing, accuracy_calculator.py:183-231,
    never looks at the distances once the order is known).  With one rank the distance row is then not written at all
    (41 instead of 50 us at 2048 x 25,000, k = 5000); the merge of the multi-rank path writes it either way."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        out = H.hamming_topk(q_local, db_shard, nbits, k, workspace=workspace, want_dist=want_dist)
        return (out[0], out[1], None) if return_need else out
    rank = dist.get_rank(group)
    lo, hi, per = shard_bounds(n_total, world, rank)
    n_local = hi - lo
    kin = min(k, per)                                   # longest list a shard could have to send
    k_local = min(kin, n_local)
    # 1. every rank needs every query
    q_all = _gather_rows(q_local, world, group)
    if not isinstance(db_shard, H.PreparedDB) and db_shard.shape[0] != n_local:
        raise ValueError(f"rank {rank}: shard has {db_shard.shape[0]} rows, expected rows [{lo}, {hi}) of {n_total}")
    nq, dev = q_all.shape[0], q_local.device
    # 2. the shard step.  Shards the windowed kernel takes never rank more than the prefix that can matter, and write it
    # straight in the 16-bit wire format: in ONE pass with the complete histograms when the prefix length is known (hinted
    # steady state: 3 collectives per step instead of 5), else histograms first -- cheap, no list -- and the lists once the
    # exchange is sized.  Any other shard ranks its k_local nearest rows in one step.
    windowed = trim and per <= H.SHARD_ROWS_MAX
    hinted = windowed and send_hint is not None
    send = _prefix_len(kin, send_hint) if hinted else kin
    rows = lists = cum = need = None
    if hinted:
        if n_local:
            rows, cum = H.hamming_shard_prefix(q_all, db_shard, nbits, min(send, n_local), workspace=workspace)
        else:                                           # empty shard: contributes nothing
            rows = torch.zeros((nq, send), dtype=torch.int16, device=dev)
    elif windowed and n_local:
        cum = H.hamming_hist(q_all, db_shard, nbits, workspace=workspace)
    elif k_local and trim:
        # the compact exchange ships histograms, not distance rows: do not even write them
        *lists, cum = H.hamming_topk(q_all, db_shard, nbits, k_local, idx_offset=lo, workspace=workspace,
                                     want_dist=per > 65536, want_cum=True)
    elif k_local:
        lists = H.hamming_topk(q_all, db_shard, nbits, k_local, idx_offset=lo, workspace=workspace)
    if trim and cum is None:                            # empty shard: contributes nothing
        cum = torch.zeros((nq, nbits + 2), dtype=torch.int32, device=dev)
    # 3. size the exchange
    if trim and not hinted:
        send, need = _exact_send(cum, k, kin, group, send_hint)
    # 4. exchange and merge
    if trim and per <= 65536:
        if windowed and n_local and rows is None:
            rows = H.hamming_topk_rows16(q_all, db_shard, nbits, min(send, n_local), workspace=workspace)
        elif rows is None:
            rows = torch.zeros((nq, send), dtype=torch.int16, device=dev)
            if lists is not None:
                w = min(send, k_local)
                rows[:, :w] = (lists[0][:, :w] - lo).to(torch.int16)   # wraps for rows >= 32768; the kernel reads uint16
        idx, d, owed = _exchange_compact(rows, cum, send, world, per, k, nbits, group, report_need=hinted)
        need = owed if hinted else need
    else:
        idx, d = _exchange_wide(lists, nq, send, world, k, nbits, dev, group)
    return (idx, d, need) if return_need else (idx, d)


def sharded_hamming_map_at_k(q_local, qlab_local, db_shard, labels_shard, nbits, k, n_total, send_hint, group=None):
    """mAP@k ingredients of THIS rank's queries against the row-sharded database, without a single list on the wire:
    -> (ap float32 [Ql], nrel int32 [Ql], need int32 [1]) or None when the shape is outside the kernels (the caller then
    uses sharded_hamming_topk + map_at_k: same numbers).

    calculate_maphashing (accuracy_calculator.py:183-231) needs of a list entry only whether it is relevant.  So a shard
    ranks every query against its rows as before, but what it sends per query is the RELEVANCE STRING of its `send_hint`
    nearest rows (1 bit per entry; the shard knows its rows' labels, the queries' label words travel with their codes in
    the one all_gather) plus its cumulative histogram; the receiver interleaves the strings bin by bin and evaluates the
    merged string exactly as map_at_k evaluates a list.  Per step: one all_gather, one ranking pass per shard, ONE small
    all_to_all (histogram and string side by side: 264 + 136 bytes per query and shard at 8 GPUs instead of 264 + 2,128 in
    two), one merge kernel.
    q_local int64 [Ql, words]; qlab_local int64 [Ql, 1 or 2] (up to 128 classes: MIRFLICKR's 38 in one label word, COCO's 80
    in two); db_shard PreparedDB and labels_shard PreparedLabels of this rank's rows; send_hint: the prefix length (learn it
    from an earlier batch, check the returned `need` with exchange_ok), or None for a one-off call that sizes the exchange
    exactly first: a histogram pass per shard, one SUM and one MAX all-reduce and one host read (what evaluate_sharded
    uses) -- `need` is then <= the prefix that was sent by construction.
    k may be a sequence of cut-offs (any order): ap and nrel are then [Ql, len(k)], column i what the call returns for k[i];
    still one all_gather and one all_to_all, their length from max(k), and `need` refers to max(k)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    multi = isinstance(k, (tuple, list))                 # several cut-offs: ap / nrel are [Ql, len(k)]
    if multi:
        k = [int(x) for x in k]
        if not k:
            raise ValueError("sharded_hamming_map_at_k: empty k sequence")
    kmax = max(k) if multi else k                        # ranking, prefix length and exchange are sized by the largest
    if world == 1:
        out = (H.hamming_map_at_ks if multi else H.hamming_map_at_k)(q_local, db_shard, labels_shard, qlab_local, nbits, k)
        return None if out is None else (out[0], out[1], None)
    rank = dist.get_rank(group)
    Ql, words = q_local.shape
    lo, hi, per = shard_bounds(n_total, world, rank)
    n_local = hi - lo
    lwords = qlab_local.shape[1]                         # 1 label word (<= 64 classes) or 2 (COCO's 80, NUS-WIDE's 81)
    if per > H.SHARD_ROWS_MAX or min(kmax, per) > H.RANK_K_MAX or lwords not in (1, 2) or nbits > 128:
        return None                                      # decided from values every rank shares: no rank goes another way
    if (multi and len(set(k)) > H.MAX_CUTOFFS) or H.merge_relbits_lds_bytes(world, kmax, nbits) > H.MERGE_LDS_LIMIT:
        return None                                      # likewise: world, max(k) and nbits are the same on every rank
    dev = q_local.device
    both_all = _gather_rows(torch.cat([q_local, qlab_local], dim=1), world, group)   # codes | label words: one collective
    q_all, ql_all = both_all[:, :words].contiguous(), both_all[:, words:words + lwords].contiguous()
    kin = min(kmax, per)
    if send_hint is None:                                # one-off call: a histogram pass, then the exact sizing
        cum = (H.hamming_hist(q_all, db_shard, nbits) if n_local > 0
               else torch.zeros((world * Ql, nbits + 2), dtype=torch.int32, device=dev))
        send = _exact_send(cum, kmax, kin, group)[0]
    else:
        send = _prefix_len(kin, send_hint)
    wire = torch.zeros((world * Ql, H.relbits_wire_words(send, nbits)), dtype=torch.int64, device=dev)
    if n_local > 0:
        got = H.hamming_shard_relbits(q_all, db_shard, labels_shard, ql_all, nbits, min(send, n_local), wire=wire, kin=send)
        if got is None:
            raise RuntimeError("sharded_hamming_map_at_k: this shard is outside the fused kernel although the shared checks passed")
        wire = got
    wire_r = torch.empty_like(wire)
    _all_to_all(wire_r, wire, group)                      # histogram + relevance string of a (query, shard) side by side
    need = torch.zeros(1, dtype=torch.int32, device=dev)
    got = (H.merge_relbits_map_ks if multi else H.merge_relbits_map)(wire_r.view(world, Ql, -1), send, k, nbits, need_out=need)
    if got is None:
        raise RuntimeError("sharded_hamming_map_at_k: the merged string does not fit although the shared checks passed")
    return got[0], got[1], need


def sharded_hamming_radius_hist(q_local, qlab_local, db_shard, labels_shard, nbits, group=None):
    """Radius histograms (H.hamming_radius_hist) of ALL ranks' queries against the row-sharded database, the same on every
    rank -> (cum, cumrel) int32 [world * Ql, nbits + 2], query rows in rank order.  The tables count disjoint row sets, so
    the shards' tables simply add: one all_gather (query codes and label words in one buffer), one pass over the shard, ONE
    SUM all_reduce of both tables -- no prefix negotiation, no merge.  Feed engine.radius_metrics with the result.
    q_local int64 [Ql, words], qlab_local int64 [Ql, 1 or 2] (every rank the same Ql); db_shard / labels_shard: this rank's
    rows as PreparedDB / PreparedLabels, or -- host tensors (gloo) -- packed int64 codes and label words, which take the
    library's host twin.  A shard may be ragged or empty."""
    from .engine import hamming_host as HH
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    Ql, words = q_local.shape
    lwords = qlab_local.shape[1]
    if lwords not in (1, 2) or nbits > 128:
        raise ValueError(f"sharded_hamming_radius_hist: 1 or 2 label words and nbits <= 128 (got {lwords}, {nbits})")
    dev = q_local.device
    both_all = torch.cat([q_local, qlab_local], dim=1).contiguous()          # codes | label words: one collective
    if world > 1:
        both_all = _gather_rows(both_all, world, group)
    q_all, ql_all = both_all[:, :words].contiguous(), both_all[:, words:].contiguous()
    tables = torch.zeros((2, world * Ql, nbits + 2), dtype=torch.int32, device=dev)
    n_local = db_shard.N if hasattr(db_shard, "N") else db_shard.shape[0]
    if n_local > 0 and Ql > 0:
        got = (H if dev.type == "cuda" else HH).hamming_radius_hist(q_all, db_shard, labels_shard, ql_all, nbits)
        if got is None:
            raise RuntimeError("sharded_hamming_radius_hist: this shard is outside the radius histograms")
        tables[0], tables[1] = got
    if world > 1:
        _all_reduce(tables, dist.ReduceOp.SUM, group)
    return tables[0], tables[1]


def exchange_ok(needs, send_hint, kin):
    """True when every `need` a hinted call returned fits the prefix length that was exchanged (one host read for
    the whole list; call it where the host synchronises anyway)."""
    needs = [n for n in needs if n is not None]
    if not needs:
        return True
    # the merge kernels report max_g cum[g][T+1] unclamped; a shard never owes more than `kin` = min(k, shard rows) entries
    # (with many ties at the k-th distance the raw count exceeds it although `kin` entries were exchanged: exact)
    worst = min(int(torch.stack([n.reshape(()) for n in needs]).max().item()), int(kin))
    return worst <= _prefix_len(kin, send_hint)


def merge_knn_lists(vals, gidx, k, metric):
    """Merge of per-shard k-NN lists -- what faiss' sharded index does on the host (get_knn.py:41-44) -- on the device the
    lists live on.  vals float32 [G, Ql, kk]: every shard's list per query, in ITS ranking order, as inner products
    (WV_METRIC_IP) or SQUARED distances (both L2 metrics); gidx int32 [G, Ql, kk]: global row numbers; padding entries of a
    short shard carry the sentinel (-inf for IP, +inf for L2).  Laid side by side in shard order, candidates with equal values
    are in ascending global row order (a shard ranks ties by ascending row, shard s holds lower rows than shard s + 1), so
    ranking the candidate matrix with ties by ascending column (wv_rank_scores) gives exactly the unsharded list.
    -> (values [Ql, k], global rows int32 [Ql, k])."""
    from . import _lib
    from .engine.get_knn import rank_scores
    G, Ql, kk = vals.shape
    cand = vals.permute(1, 0, 2).reshape(Ql, G * kk).contiguous()
    rows = gidx.permute(1, 0, 2).reshape(Ql, G * kk)
    v, pos = rank_scores(cand, k, descending=metric == _lib.WV_METRIC_IP, sqrt=metric == _lib.WV_METRIC_L2)
    return v, torch.gather(rows, 1, pos.long())


def sharded_knn_float(q_local, db_shard, k, metric, n_total, group=None):
    """Real-valued k-NN over a row-sharded database, one process per GPU: the role faiss.index_cpu_to_all_gpus(shards=True)
    plays for IndexFlatIP / IndexFlatL2 in the reference (main/engine/get_knn.py:35-52).  q_local [Ql, D]: THIS rank's
    queries (every rank the same Ql); db_shard: rows [rank * per, ...) of the database, per = ceil(n_total / world).
    One all_gather of the queries, wv_knn_float on the shard for everybody's queries, one all_to_all of the per-shard lists
    (value bits and global row packed into 8 bytes per entry), merge_knn_lists.  Results are those of wv_knn_float on the
    whole database, bit for bit, for every world size.  Host tensors (gloo) take the library's host twins.
    -> (values [Ql, k], global rows int32 [Ql, k])."""
    from . import _lib
    from .engine.backend import backend
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, _, per = shard_bounds(n_total, world, rank)
    if k > n_total:
        raise RuntimeError(f"selected index k out of range (k={k}, references={n_total})")
    q_local = q_local.float().contiguous()
    Ql, D = q_local.shape
    dev = q_local.device
    q_all = torch.empty((world * Ql, D), dtype=torch.float32, device=dev)
    if world > 1:
        _all_gather(q_all, q_local, group)
    else:
        q_all.copy_(q_local)
    kk = min(k, per)
    n_loc = db_shard.shape[0]
    shard_metric = _lib.WV_METRIC_IP if metric == _lib.WV_METRIC_IP else _lib.WV_METRIC_L2_SQUARED
    sentinel = float("-inf") if metric == _lib.WV_METRIC_IP else float("inf")
    vals = torch.full((world * Ql, kk), sentinel, dtype=torch.float32, device=dev)
    rows = torch.full((world * Ql, kk), -1, dtype=torch.int32, device=dev)
    k_loc = min(kk, n_loc)
    if k_loc:
        v, i = backend(dev).knn_float(db_shard, q_all, k_loc, shard_metric)
        vals[:, :k_loc] = v
        rows[:, :k_loc] = i + lo
    # one 8-byte word per entry: value bits | global row
    send = (vals.view(torch.int32).long() << 32) | (rows.long() & 0xFFFFFFFF)
    recv = torch.empty_like(send)
    if world > 1:
        _all_to_all(recv, send.contiguous(), group)      # [shard, Ql, kk] of this rank's queries
    else:
        recv = send
    recv = recv.view(world, Ql, kk)
    got_v = (recv >> 32).int().view(torch.float32)
    got_i = (recv & 0xFFFFFFFF).int()
    return merge_knn_lists(got_v, got_i, k, metric)
