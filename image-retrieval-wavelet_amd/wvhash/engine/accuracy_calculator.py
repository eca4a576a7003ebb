"""GPU accuracy calculator with the method surface of
/root/reference/main/engine/accuracy_calculator.py (CustomCalculator :16-349,
get_accuracy_calculator :352-403).

The reference subclasses pytorch_metric_learning's AccuracyCalculator and runs on CPU tensors; this
class is self-contained (PML is not a dependency), keeps everything on the GPU -- or, with an explicit ``device='cpu'`` (the
reference's own configuration, main/engine/evaluate.py:76-81; BASELINE config c0), on the host through the `_cpu` twins
of the same entry points (csrc/host_rank.cpp; same integers, same AP bits) -- and routes the arithmetic through libwvhash:
  calc_hamming_dist       -> wv_hamming_dist        (:183-186)
  calculate_maphashing    -> wv_hamming_map_at_k, or wv_hamming_topk + wv_map_at_k   (:203-231, the reported metric)
                             with soft_codes = True and embeddings that are not +-1 (the batch mAP proxy, engine/batch_map.py)
                             -> wv_ip_map_at_k, or wv_knn_float + wv_map_at_k
  calculate_maphashing_at -> wv_hamming_map_at_ks / wv_map_at_ks: the same at several cut-offs from one ranking pass
  calculate_bit_balance / calculate_worst_bit_balance -> wv_bit_counts   (:188-200)
  calculate_map           -> get_knn + wv_map_at_k  (:156-167, torchmetrics RetrievalMAP)
  calculate_rpr / calculate_pr / calculate_pr_rc / calculate_pr_rc_hashing -> wv_hit_prefix (:131-181, :235-273)
  calculate_precision_hamming_radius / calculate_pr_curve_hamming (opt-in: computed only when named in `include`)
                          -> wv_hamming_radius_hist (DSCH/_utils.py:469-493, 577-594: precision / recall by Hamming radius)
  calculate_ndcg_hamming (opt-in likewise) -> wv_label_overlap_hist + wv_ndcg_at_ks (DSCH/_utils.py:551-574: NDCG@ndcg_k)
Ranking ties are broken by ascending reference index (see engine/get_knn.py).

Two decisions have one place each.  Where it runs: engine/backend.py maps `device` to the primitives module, the tensor move
and the float k-NN.  How a (query, reference) pair is packed, prepared and ranked: RankCache, the ranking session.  Every metric
is one body over a session -- the shared one when `rank_cache=` was given, otherwise one made for that metric call and dropped
with it, so that no list outlives the call.
"""
import logging

import torch

from .. import _lib
from . import ndcg as ndcg_metrics
from . import radius_metrics
from .backend import HOST, backend
from .get_knn import get_knn, _is_pm1
from .hamming import SHARD_ROWS_MAX

LOGGER = logging.getLogger("RETRIEVAL")

_RECALL_KS = (1, 2, 4, 8, 10, 16, 20, 30, 32, 100, 1000)
_NOT_METRICS = ("calculate_maphashing_at",)     # calculate_* methods that take cut-offs of their own: not get_accuracy columns
_OPT_IN = ("precision_hamming_radius", "pr_curve_hamming", "ndcg_hamming")   # computed only when `include` names them (construction or get_accuracy)


class RankCache(object):
    """The ranking session of ONE (query, reference) embedding pair on one backend (`device` as in CustomCalculator): packed
    codes, packed labels, the prepared database and its labels, ranked lists and AP columns, each made once.  Shared by the
    calculators of an evaluate_multi_k run it ranks once at the largest k asked for and every smaller k reads a prefix (the
    reference re-runs its whole per-query loop for every k, main/engine/evaluate.py:226-243).
    Entries are keyed by tensor identity (storage pointer, shape, version counter): new embeddings invalidate them."""

    def __init__(self, kmax_hint=0, ks=(), device=None):
        self.backend = backend(device)
        self.ks = sorted({int(k) for k in ks if isinstance(k, int) and not isinstance(k, bool) and k > 0})   # the run's cut-offs
        self.kmax_hint = max([int(kmax_hint)] + self.ks)
        self._codes, self._labels, self._lists, self._aps, self._db, self._dblabels = {}, None, None, None, None, None

    @staticmethod
    def _key(t):
        return (t.data_ptr(), tuple(t.shape), t.dtype, t._version)

    def packed_codes(self, x, key=None):
        key = key or self._key(x)
        if key not in self._codes:
            self._codes = {k_: v for k_, v in self._codes.items() if len(self._codes) < 4}
            self._codes[key] = self.backend.H.pack_codes(x)
        return self._codes[key]

    def packed_labels(self, query_labels, reference_labels, key=None):
        key = key or (self._key(query_labels), self._key(reference_labels))
        if self._labels is None or self._labels[0] != key:
            if query_labels.ndim == 1:  # class-id labels: one-hot them onto bits
                classes = torch.unique(torch.cat([query_labels, reference_labels]))
                query_labels = (query_labels.unsqueeze(1) == classes).float()
                reference_labels = (reference_labels.unsqueeze(1) == classes).float()
            H = self.backend.H
            self._labels, self._dblabels = (key, (H.pack_labels(query_labels), H.pack_labels(reference_labels))), None
        return self._labels[1]

    def _prepared_db(self, reference, make=True, key=None):
        """PreparedDB of the reference set, laid out once per embedding pair (make=False: None when there is none yet)."""
        key = key or self._key(reference)
        if self._db is not None and self._db[0] == key:
            return self._db[1]
        if make:
            self._db = (key, self.backend.H.PreparedDB(self.packed_codes(reference, key), reference.shape[1]))
            return self._db[1]

    def _ranking_db(self, reference):
        """What hamming_topk ranks against: the prepared database if the session has it, a new prepared one beyond
        SHARD_ROWS_MAX rows (virtual shards through the windowed kernel; never on the host), otherwise the packed codes."""
        db = self._prepared_db(reference, make=reference.shape[0] > self.backend.H.SHARD_ROWS_MAX)
        return db if db is not None else self.packed_codes(reference)

    def _prepared_labels(self, rlp):
        """PreparedLabels of the packed reference labels this session holds."""
        if self._dblabels is None:
            self._dblabels = self.backend.H.PreparedLabels(rlp)
        return self._dblabels

    def _has_lists(self, query, reference, k, want_dist=False):
        got = self._lists
        return (got is not None and got[0] == (self._key(query), self._key(reference)) and got[1].shape[1] >= k
                and not (want_dist and got[2] is None))

    def lists(self, query, reference, k, want_dist=False):
        """int32 [Q, >= k] ranked lists (ascending distance, then index); only the first k columns are meaningful to the caller."""
        if not self._has_lists(query, reference, k, want_dist):
            db = self._ranking_db(reference)
            kk = min(reference.shape[0], max(k, self.kmax_hint))
            idx, dist = self.backend.H.hamming_topk(self.packed_codes(query), db, reference.shape[1], kk, want_dist=want_dist)
            self._lists = ((self._key(query), self._key(reference)), idx, dist)
        return self._lists[1]

    def maphashing(self, query, query_labels, reference, reference_labels, topk, also=()):
        """Average precision per query at `topk` (float32 [Q]).  The first call for an embedding pair answers ALL the run's
        cut-offs (and those in `also`: further cut-offs the caller will ask for next), MAX_CUTOFFS per pass, and keeps the
        columns.  Each pass reads the session's lists when a k-NN metric already made them; otherwise it is the fused ranking +
        AP kernel, so that no [Q, k_max] list exists; where that answers None (shape outside it; always on the host) the lists
        are ranked at the largest cut-off and read.  One cut-off takes the single-k entry points, several the multi-k ones:
        the same bits."""
        H = self.backend.H
        num_ref, nbits = reference.shape
        topk = min(int(topk), num_ref)
        key = (self._key(query), self._key(reference), self._key(query_labels), self._key(reference_labels))   # each tensor's key once
        if self._aps is None or self._aps[0] != key:
            self._aps = (key, {})
        done = self._aps[1]
        if topk not in done:
            want = sorted({min(int(k), num_ref) for k in (*self.ks, *also)} | {topk})
            qlp, rlp = self.packed_labels(query_labels, reference_labels, key[2:])
            for s in range(0, len(want), H.MAX_CUTOFFS):
                ks = want[s:s + H.MAX_CUTOFFS]
                got = None
                if not self._has_lists(query, reference, ks[-1]) and nbits <= 128 and rlp.shape[1] <= 2:
                    db, qp, labels = self._prepared_db(reference, key=key[1]), self.packed_codes(query, key[0]), self._prepared_labels(rlp)
                    got = (H.hamming_map_at_k(qp, db, labels, qlp, nbits, ks[0]) if len(ks) == 1
                           else H.hamming_map_at_ks(qp, db, labels, qlp, nbits, ks))
                if got is None:
                    idx = self.lists(query, reference, want[-1])
                    got = H.map_at_k(idx, qlp, rlp, k=ks[0]) if len(ks) == 1 else H.map_at_ks(idx, qlp, rlp, ks)
                done.update({k: got[0] if len(ks) == 1 else got[0][:, i] for i, k in enumerate(ks)})
        return done[topk]

    def ip_maphashing(self, query, query_labels, reference, reference_labels, topk):
        """Average precision per query at `topk` (float32 [Q]) of REAL-VALUED embeddings ranked by descending inner product --
        the order of the reference's key 0.5 * (nbits - q @ r.T), ties by ascending row: one launch (wv_ip_map_at_k) where
        the shape allows; where that answers None the float k-NN ranks to `topk` and map_at_k reads the list: by the entry
        point's contract the same bits."""
        H = self.backend.H
        qlp, rlp = self.packed_labels(query_labels, reference_labels)
        got = H.ip_map_at_k(query, reference, qlp, rlp, topk)
        if got is None:
            _, idx = self.backend.knn_float(reference, query, topk, _lib.WV_METRIC_IP)
            got = H.map_at_k(idx, qlp, rlp, k=topk)
        return got[0]

    def map_at_k(self, idx, query_labels, reference_labels, k=None):
        """(ap, nrel) of lists the caller ranked (k-NN lists), over the session's packed labels."""
        return self.backend.H.map_at_k(idx, *self.packed_labels(query_labels, reference_labels), k=k)

    def hit_prefix(self, idx, query_labels, reference_labels):
        """Running hit counts along the ranked lists, int32 [Q, k] (wv_hit_prefix)."""
        return self.backend.H.hit_prefix(idx.int(), *self.packed_labels(query_labels, reference_labels))

    def radius_tables(self, query, query_labels, reference, reference_labels):
        """(cum, cumrel) of hamming_radius_hist for the pair, from the packed codes / labels and the prepared database."""
        qlp, rlp = self.packed_labels(query_labels, reference_labels)
        qp = self.packed_codes(query)
        return self.backend.H.hamming_radius_hist(qp, self._prepared_db(reference), self._prepared_labels(rlp), qlp, reference.shape[1])

    def ndcg_sums(self, query, query_labels, reference, reference_labels, k):
        """(dcg, idcg) float64 [Q, 1] at cut-off k: from the session's lists when they reach k, otherwise from lists ranked
        chunk by chunk (ndcg.LIST_BYTES_MAX) and dropped."""
        H = self.backend.H
        qlp, rlp = self.packed_labels(query_labels, reference_labels)
        if self._has_lists(query, reference, k):
            lists_of = lambda lo, hi: self._lists[1][lo:hi]
        else:
            qp, db, nbits = self.packed_codes(query), self._ranking_db(reference), reference.shape[1]
            lists_of = lambda lo, hi: H.hamming_topk(qp[lo:hi], db, nbits, k, want_dist=False)[0]
        return ndcg_metrics.ndcg_sums_packed(H, lists_of, query.shape[0], qlp, rlp, [k])

    def knn(self, reference, query, num_k, same_source):
        """get_knn(..., distance_metric='hamming') from the session's ranking: (indices int64, inner products fp32)."""
        num_k += int(same_source)
        if num_k > reference.shape[0]:
            raise RuntimeError(f"selected index k out of range (k={num_k}, references={reference.shape[0]})")
        idx = self.lists(query, reference, num_k, want_dist=True)[:, :num_k]
        ip = float(reference.shape[1]) - 2.0 * self._lists[2][:, :num_k].float()
        first = int(same_source)
        return idx[:, first:].long(), ip[:, first:]


class CustomCalculator(object):

    def __init__(self, include=(), exclude=(), avg_of_avgs=False, return_per_class=False, k=None,
                 label_comparison_fn=None, device=None, knn_func=None, kmeans_func=None,
                 with_faiss=True, distance_metric="l2", **kwargs):
        if label_comparison_fn is not None or knn_func is not None or kmeans_func is not None:
            raise NotImplementedError("custom label_comparison_fn / knn_func / kmeans_func are not supported")
        if avg_of_avgs or return_per_class:
            raise NotImplementedError("avg_of_avgs / return_per_class are not supported")
        if not (isinstance(k, int) and k > 0) and k not in (None, "max_bin_count"):
            raise ValueError("k must be a positive int, None or 'max_bin_count'")
        self.k = k
        self.num_top_k = k
        self.with_faiss = with_faiss
        self.pr_rc_path, self.last_pr_rc = kwargs.pop("pr_rc_path", "pr_rc.csv"), None
        self.hamming_radius = kwargs.pop("hamming_radius", 2)
        self.ndcg_k = kwargs.pop("ndcg_k", 1000)                  # the reference's call: NDCG(qB, rB, qL, rL, what=1, k=1000)
        self.pr_curve_hamming_path, self.last_pr_curve_hamming = kwargs.pop("pr_curve_hamming_path", None), None
        self.distance_metric = distance_metric
        self.rank_cache = kwargs.pop("rank_cache", None)          # shared by the calculators of evaluate_multi_k
        # False: calculate_maphashing takes +-1 codes only (anything else raises in the packer).  True: embeddings that are
        # not exactly +-1 are ranked by inner product like the reference's calc_hamming_dist ranks them (wv_ip_map_at_k);
        # +-1 codes take the packed path either way.  build_batch_map_calculator sets it.
        self.soft_codes = False
        # device=None / 'cuda': the ranking stage lives on the GPU.  device='cpu' (what the reference pins its calculator
        # to, main/engine/evaluate.py:76-81): the host twins of the same entry points -- explicit, never a fallback: without
        # a GPU and without device='cpu' every metric raises WvhashUnavailable.
        self.requested_device = device
        self.backend = backend(device)
        self.host = self.backend is HOST
        self._dev = self.backend.move       # tensor on the calculator's device (accuracy_calculator.py:290-293 moves everything to self.device)
        if self.rank_cache is not None and self.rank_cache.backend is not self.backend:
            side, own = ("GPU", "cpu") if self.host else ("host", "cuda")
            raise ValueError(f"a shared RankCache holds {side} lists: not available with device='{own}'")
        self.original_function_dict = {name[len("calculate_"):]: getattr(self, name)
                                       for name in dir(self) if name.startswith("calculate_") and name not in _NOT_METRICS}
        self.check_primary_metrics(include, exclude)
        every = self.original_function_dict
        self._opted_in = tuple(m for m in _OPT_IN if m in include and m not in exclude)
        self.original_function_dict = self.get_function_dict(include, exclude)
        # the opt-in metrics stay nameable in get_accuracy(include=...); an empty include never selects them
        self.original_function_dict.update({m: every[m] for m in _OPT_IN if m not in exclude})
        self.curr_function_dict = self.get_function_dict()
        LOGGER.info(f"Initializing CustomCalculator with with_faiss={with_faiss} and "
                    f"distance_metric={distance_metric} device: {'cpu (host twins)' if self.host else 'cuda (HIP)'}")

    # ------------------------------------------------------------------ bookkeeping (PML surface)
    @property
    def device(self):
        if self.host:
            return torch.device("cpu")
        _lib.require_gpu()
        return torch.device("cuda", torch.cuda.current_device())

    def _session(self, throw_away=True):
        """The ranking session a metric talks to: the shared one, or (throw_away) one of its own that is dropped with the
        metric call, lists and all."""
        if self.rank_cache is not None:
            return self.rank_cache
        return RankCache(device=self.requested_device) if throw_away else None

    def check_primary_metrics(self, include=(), exclude=()):
        # unlike PML, names this implementation does not compute are tolerated in `exclude`
        # (the reference's exclude lists name PML metrics such as NMI / AMI / mean_reciprocal_rank)
        for m in include:
            if m not in self.original_function_dict:
                raise ValueError(f"{m} is not a metric computed by wvhash; valid: {sorted(self.original_function_dict)}")

    def get_function_dict(self, include=(), exclude=()):
        if len(include) == 0:
            opted = getattr(self, "_opted_in", ())
            include = [k for k in self.original_function_dict.keys() if k not in _OPT_IN or k in opted]
        included = [k for k in include if k not in exclude]
        return {k: v for k, v in self.original_function_dict.items() if k in included}

    def get_curr_metrics(self):
        return [k for k in self.curr_function_dict.keys()]

    def requires_knn(self):
        return ["precision_at_1", "recall_classic", "rpr", "pr", "pr_rc", "map"] + \
               [f"recall_at_{k}" for k in _RECALL_KS]

    def requires_clustering(self):
        return []

    def description(self):
        return "avg_of_avgs" if False else ""

    def determine_k(self, bin_counts, num_reference_embeddings, embeddings_come_from_same_source):
        self_count = int(embeddings_come_from_same_source)
        if self.k == "max_bin_count":
            return int(torch.max(bin_counts).item()) - self_count
        if self.k is None:
            return num_reference_embeddings - self_count
        return self.k

    # ------------------------------------------------------------------ relevance (:31-37)
    def label_comparison_fn(self, query_labels, reference_labels):
        if query_labels.ndim > 1 and reference_labels.ndim > 1:
            if query_labels.dim() == 2 and reference_labels.dim() == 2:
                return torch.matmul(query_labels.float(), reference_labels.t().float()) > 0
            return (query_labels.float() * reference_labels.float()).sum(dim=-1) > 0
        return query_labels.unsqueeze(1) == reference_labels

    def _match_counts(self, query_labels, reference_labels, chunk=256):
        """#references relevant to each query (what PML's get_label_match_counts feeds determine_k /
        the lone-query mask with), chunked so the [Q, N] relevance matrix is never whole in memory."""
        out = torch.empty(query_labels.shape[0], dtype=torch.long, device=query_labels.device)
        for s in range(0, query_labels.shape[0], chunk):
            out[s:s + chunk] = self.label_comparison_fn(query_labels[s:s + chunk], reference_labels).sum(dim=1)
        return out

    # ------------------------------------------------------------------ hashing primitives
    def calc_hamming_dist(self, qB, rB):
        """0.5 * (B - qB @ rB.T) for +-1 codes (:183-186) -> fp32 [Q, N] like the reference."""
        qB, rB = self._dev(qB), self._dev(rB)
        H = self.backend.H
        return H.hamming_dist(H.pack_codes(qB), H.pack_codes(rB), nbits=qB.shape[1]).float()

    def per_bit_balance(self, reference):
        reference = self._dev(reference)
        nbits = reference.shape[1]
        counts = self.backend.H.bit_counts(self.backend.H.pack_codes(reference, check=False), nbits)
        frac_positive = counts.float() / float(reference.shape[0])
        return 1.0 - 2.0 * (frac_positive - 0.5).abs()

    def calculate_bit_balance(self, reference, **kwargs):
        return self.per_bit_balance(reference).mean().item()

    def calculate_worst_bit_balance(self, reference, **kwargs):
        return self.per_bit_balance(reference).min().item()

    def _average_precisions(self, idx, query_labels, reference_labels, k=None):
        return self._session().map_at_k(idx, query_labels, reference_labels, k=k)

    def _hits(self, idx, query_labels, reference_labels):
        """Running hit counts along the ranked lists, int32 [Q, k] (wv_hit_prefix)."""
        return self._session().hit_prefix(idx, query_labels, reference_labels)

    def calculate_maphashing(self, query, query_labels, reference, reference_labels, topk,
                             ref_includes_query=False, return_per_query=False, **kwargs):
        while isinstance(topk, (tuple, list)):
            topk = topk[0] if len(topk) else None
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)
        if topk == "max_bin_count":
            topk = int(self._match_counts(reference_labels, reference_labels).max().item()) - int(ref_includes_query)
        num_ref = reference.shape[0]
        topk = num_ref if topk is None else min(int(topk), num_ref)  # gnd[0:topk] clips at N
        num_query = query.shape[0]
        if num_query == 0:
            raise ZeroDivisionError("calculate_maphashing: no queries")
        if self.soft_codes and topk <= 0:
            # a same-source batch in which no two rows share a tag: the reference's gnd[0:0] is empty, every AP is 0 -- no launch
            return (0.0, torch.zeros(num_query, dtype=torch.float32, device=query.device)) if return_per_query else 0.0
        if self.soft_codes and not (_is_pm1(reference) and (query is reference or _is_pm1(query))):
            # real-valued embeddings (tanh values, BN logits): the reference's own key on them, no packing
            ap = self._session().ip_maphashing(query, query_labels, reference, reference_labels, topk)
        else:
            # ranking and AP in one kernel where the shape allows and no list exists yet; otherwise lists, then AP (same numbers)
            ap = self._session().maphashing(query, query_labels, reference, reference_labels, topk)
        result = ap.double().sum().item() / num_query
        if return_per_query:
            return result, ap
        return result

    def calculate_maphashing_at(self, query, query_labels, reference, reference_labels, ks, ref_includes_query=False,
                                return_per_query=False, **kwargs):
        """calculate_maphashing at several cut-offs from ONE ranking pass -> {k: value} (return_per_query: {k: (value, ap
        float32 [Q])}), each value what calculate_maphashing returns for topk = k.  ks: positive ints in any order, repeats
        allowed; a cut-off beyond the reference set clips at its size like gnd[0:topk]."""
        ks = list(ks)
        if not ks or not all(isinstance(k, int) and not isinstance(k, bool) and k > 0 for k in ks):
            raise ValueError("calculate_maphashing_at: ks must be a non-empty sequence of positive ints")
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)
        num_query, num_ref = query.shape[0], reference.shape[0]
        if num_query == 0:
            raise ZeroDivisionError("calculate_maphashing_at: no queries")
        eff = [min(k, num_ref) for k in ks]
        session = self._session()
        if self.soft_codes and not (_is_pm1(reference) and (query is reference or _is_pm1(query))):
            # real-valued embeddings: one wv_ip_map_at_k call per cut-off
            cols = {k: session.ip_maphashing(query, query_labels, reference, reference_labels, k) for k in set(eff)}
        else:
            cols = {k: session.maphashing(query, query_labels, reference, reference_labels, k, also=eff) for k in eff}
        out = {}
        for k, ke in zip(ks, eff):
            value = cols[ke].double().sum().item() / num_query
            out[k] = (value, cols[ke]) if return_per_query else value
        return out

    # ------------------------------------------------------------------ knn metrics
    def calculate_map(self, query_labels, knn_indices, reference_labels, not_lone_query_mask, **kwargs):
        """RetrievalMAP over the k-NN lists (:156-167): AP per kept query, no-hit queries count 0."""
        ap, _ = self._average_precisions(knn_indices.int(), query_labels, reference_labels)
        kept = ap[not_lone_query_mask]
        return kept.double().mean().item() if kept.numel() else 0.0

    def calculate_rpr(self, query_labels, knn_indices, reference_labels, not_lone_query_mask, **kwargs):
        """RetrievalRPrecision over the k-NN lists (:131-142): relevant among the first R / R, R = relevant
        entries of the list; lists in k-NN order (ties: ascending reference index)."""
        hits = self._hits(knn_indices, query_labels, reference_labels)[not_lone_query_mask].long()
        if not hits.numel():
            return 0.0
        R = hits[:, -1]
        top = torch.gather(hits, 1, (R - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
        return torch.where(R > 0, top.double() / R.clamp(min=1).double(), torch.zeros_like(R, dtype=torch.float64)) \
            .mean().item()

    def calculate_pr(self, query_labels, knn_indices, reference_labels, not_lone_query_mask, **kwargs):
        """RetrievalPrecision(top_k=1) (:144-154)."""
        first = self._hits(knn_indices[:, :1], query_labels, reference_labels)[not_lone_query_mask]
        return first.double().mean().item() if first.numel() else 0.0

    def _curves(self, hits):
        """precision@j, recall@j (j = 1..k) averaged over the rows of `hits`; rows without a hit count zero."""
        h = hits.double()
        tot = h[:, -1:]
        j = torch.arange(1, h.shape[1] + 1, dtype=torch.float64, device=h.device)
        has = tot > 0
        prec = torch.where(has, h / j, torch.zeros_like(h)).mean(0)
        rec = torch.where(has, h / tot.clamp(min=1), torch.zeros_like(h)).mean(0)
        return prec, rec

    def _write_pr_rc(self, prec, rec):
        self.last_pr_rc = (prec, rec)
        if self.pr_rc_path:                           # the reference writes ./pr_rc.csv as a side effect
            import pandas as pd
            pd.DataFrame({"pr": prec.cpu().numpy(), "rc": rec.cpu().numpy()}).to_csv(self.pr_rc_path, index=False)

    def calculate_pr_rc(self, query_labels, knn_indices, reference_labels, not_lone_query_mask, **kwargs):
        """RetrievalPrecisionRecallCurve over the k-NN lists (:169-181): writes the curve, returns 0."""
        hits = self._hits(knn_indices, query_labels, reference_labels)[not_lone_query_mask]
        if hits.numel():
            self._write_pr_rc(*self._curves(hits))
        return 0

    def calculate_pr_rc_hashing(self, query, query_labels, reference, reference_labels, not_lone_query_mask=None,
                                **kwargs):
        """Full-gallery precision / recall curves along the Hamming ranking (:235-273), averaged over the
        queries that are not lone and have a relevant item; writes the curve, returns 0."""
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)
        session, num_ref = self._session(), reference.shape[0]
        hits = session.hit_prefix(session.lists(query, reference, num_ref)[:, :num_ref], query_labels, reference_labels)
        ok = hits[:, -1] > 0
        if not_lone_query_mask is not None:
            ok &= not_lone_query_mask
        if bool(ok.any()):
            self._write_pr_rc(*self._curves(hits[ok]))
        return 0

    # ------------------------------------------------------------------ by Hamming radius (DSCH/_utils.py:469-493, 577-594)
    def _radius_tables(self, query, query_labels, reference, reference_labels):
        """(cum, cumrel) int32 [Q, nbits + 2] of the pair (wv_hamming_radius_hist, its host twin with device='cpu')."""
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)
        nbits = reference.shape[1]
        if query.dim() != 2 or query.shape[1] != nbits or nbits > 128 or not (_is_pm1(query) and _is_pm1(reference)):
            raise ValueError("Hamming-radius metrics need +-1 codes of at most 128 bits "
                             f"(got {tuple(query.shape)} / {tuple(reference.shape)})")
        got = self._session().radius_tables(query, query_labels, reference, reference_labels)
        if got is None:
            raise ValueError("Hamming-radius metrics need labels of at most 128 classes and a database of at most "
                             f"{64 * SHARD_ROWS_MAX} rows on the GPU (got {tuple(reference_labels.shape)} labels, "
                             f"{reference.shape[0]} rows)")
        return got

    def calculate_precision_hamming_radius(self, query, query_labels, reference, reference_labels, **kwargs):
        """Precision of a lookup within Hamming radius `hamming_radius` (constructor kwarg, 2 = P@H<=2), mean over all
        queries: get_precision_recall_by_Hamming_Radius (DSCH/_utils.py:577-594).  Opt-in: name it in `include`."""
        if query.shape[0] == 0:
            raise ZeroDivisionError("calculate_precision_hamming_radius: no queries")
        tables = self._radius_tables(query, query_labels, reference, reference_labels)
        return radius_metrics.precision_within_radius(*tables, radius=self.hamming_radius)

    def calculate_pr_curve_hamming(self, query, query_labels, reference, reference_labels, **kwargs):
        """Precision / recall at every Hamming radius 0..nbits (pr_curve, DSCH/_utils.py:469-493): keeps (P, R) in
        last_pr_curve_hamming, writes pr_curve_hamming_path (columns radius, pr, rc) when one is set, returns 0 -- the
        contract of calculate_pr_rc_hashing.  Opt-in: name it in `include`."""
        P, R = radius_metrics.radius_curves(*self._radius_tables(query, query_labels, reference, reference_labels))
        self.last_pr_curve_hamming = (P, R)
        if self.pr_curve_hamming_path:
            import pandas as pd
            pd.DataFrame({"radius": list(range(P.shape[0])), "pr": P.cpu().numpy(), "rc": R.cpu().numpy()}) \
                .to_csv(self.pr_curve_hamming_path, index=False)
        return 0

    # ------------------------------------------------------------------ graded relevance (DSCH/_utils.py:551-574)
    def calculate_ndcg_hamming(self, query, query_labels, reference, reference_labels, **kwargs):
        """NDCG@ndcg_k (constructor kwarg, 1000 = the reference's call; < 0 or beyond the reference set: all of it) of the
        Hamming ranking with graded relevance 2^(shared classes) - 1: what ndcg.NDCG(query, reference, query_labels,
        reference_labels, what=1, k=ndcg_k) returns for the same tensors.  Opt-in: name it in `include`."""
        if query.shape[0] == 0:
            raise ZeroDivisionError("calculate_ndcg_hamming: no queries")
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)
        (num_ref, nbits), k = reference.shape, int(self.ndcg_k)
        k = num_ref if k < 0 or k > num_ref else k
        if query.dim() != 2 or query.shape[1] != nbits or nbits > 128 or not (_is_pm1(query) and _is_pm1(reference)):
            raise ValueError(f"ndcg_hamming needs +-1 codes of at most 128 bits (got {tuple(query.shape)} / {tuple(reference.shape)})")
        if query_labels.dim() != 2 or reference_labels.dim() != 2 or query_labels.shape[1] != reference_labels.shape[1] \
                or reference_labels.shape[1] > 128 or k < 1:
            raise ValueError("ndcg_hamming needs multi-hot labels of at most 128 classes and a cut-off >= 1 "
                             f"(got {tuple(reference_labels.shape)} labels, ndcg_k={self.ndcg_k})")
        sums = self._session().ndcg_sums(query, query_labels, reference, reference_labels, k)
        return ndcg_metrics.ndcg_from_sums(*sums)[0].item()

    def _knn_relevance(self, query_labels, knn_labels, k):
        return self.label_comparison_fn(query_labels[:, None], knn_labels[:, :k]) if query_labels.ndim > 1 \
            else (query_labels[:, None] == knn_labels[:, :k])

    def recall_at_k(self, knn_labels, query_labels, k):
        return self._knn_relevance(query_labels, knn_labels, k).any(1).float().mean().item()

    def calculate_precision_at_1(self, knn_labels, query_labels, not_lone_query_mask, **kwargs):
        rel = self._knn_relevance(query_labels, knn_labels, 1)[:, 0][not_lone_query_mask]
        return rel.float().mean().item() if rel.numel() else 0.0

    # ------------------------------------------------------------------ driver (:279-349)
    def get_accuracy(self, query, query_labels, reference, reference_labels,
                     embeddings_come_from_same_source, include=(), exclude=(), return_indices=False):
        query, reference = self._dev(query), self._dev(reference)
        query_labels, reference_labels = self._dev(query_labels), self._dev(reference_labels)

        if query_labels.ndim == 1 or (query_labels.ndim == 2 and query_labels.size(1) == 1):
            query_labels = query_labels.view(-1)
            reference_labels = reference_labels.view(-1)

        self.curr_function_dict = self.get_function_dict(include, exclude)

        kwargs = {
            "query": query,
            "reference": reference,
            "query_labels": query_labels,
            "reference_labels": reference_labels,
            "embeddings_come_from_same_source": embeddings_come_from_same_source,
            "label_comparison_fn": self.label_comparison_fn,
            "ref_includes_query": embeddings_come_from_same_source,
            "topk": self.num_top_k,
        }

        knn_indices = None
        wants_knn = any(x in self.requires_knn() for x in self.get_curr_metrics())
        if wants_knn or "pr_rc_hashing" in self.get_curr_metrics():
            match_counts = self._match_counts(query_labels, reference_labels)
            not_lone_query_mask = (match_counts - int(embeddings_come_from_same_source)) > 0
            kwargs["not_lone_query_mask"] = not_lone_query_mask
        if wants_knn:
            num_k = self.determine_k(match_counts, len(reference), embeddings_come_from_same_source)
            shared = self._session(throw_away=False)     # its lists answer +-1 codes under the hamming metric
            if (shared is not None and self.distance_metric == "hamming" and reference.shape[1] <= 128
                    and _is_pm1(reference) and _is_pm1(query)):
                knn_indices, knn_distances = shared.knn(reference, query, num_k, embeddings_come_from_same_source)
            else:
                knn_indices, knn_distances = get_knn(
                    reference, query, num_k, embeddings_come_from_same_source,
                    with_faiss=self.with_faiss, distance_metric=self.distance_metric, device=self.requested_device,
                )
            if not bool(not_lone_query_mask.any()):
                LOGGER.warning("None of the query labels are in the reference set.")
            kwargs["knn_indices"] = knn_indices
            kwargs["knn_distances"] = knn_distances
            if any(m.startswith("recall_at_") or m == "precision_at_1" for m in self.get_curr_metrics()):
                kwargs["knn_labels"] = reference_labels[knn_indices[:, :1000]]

        result = self._get_accuracy(self.curr_function_dict, **kwargs)
        if return_indices:
            return knn_indices, result
        return result

    def _get_accuracy(self, function_dict, **kwargs):
        return {k: v(**kwargs) for k, v in function_dict.items()}


def _make_recall(k):
    def calculate(self, knn_labels, query_labels, **kwargs):
        return self.recall_at_k(knn_labels, query_labels, k)
    calculate.__name__ = f"calculate_recall_at_{k}"
    return calculate


for _k in _RECALL_KS:
    setattr(CustomCalculator, f"calculate_recall_at_{_k}", _make_recall(_k))


def get_accuracy_calculator(exclude_ranks=None, k=19581, with_AP=True, **kwargs):
    """Same exclude-list construction as the reference (:352-403)."""
    caller_exclude = kwargs.pop('exclude', [])
    exclude = list(caller_exclude)
    if with_AP:
        exclude.extend(['NMI', 'AMI'])
    else:
        exclude.extend(['NMI', 'AMI', 'mean_average_precision', 'mean_average_precision_at_r'])
    if exclude_ranks:
        for r in exclude_ranks:
            exclude.append(f'recall_at_{r}')
    base_exclude = [
        "mean_reciprocal_rank", "precision_at_1", "recall_at_1", "recall_at_1000", "recall_at_100",
        "recall_at_10", "recall_at_16", "recall_at_20", "recall_at_30", "recall_at_32",
        "recall_at_4", "recall_at_8", "recall_at_2", "recall_at_10", "pr_rc_hashing",
    ]
    exclude = sorted(set(exclude) | set(base_exclude))
    LOGGER.info(f"Excluding metrics: {exclude}")
    return CustomCalculator(exclude=exclude, k=k, **kwargs)
