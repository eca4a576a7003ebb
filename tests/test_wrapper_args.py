"""The argument gate in front of the C ABI of the Hamming wrappers (wvhash/engine/_args.py, used by engine/hamming.py and
engine/hamming_host.py), without a GPU: (a) the gate's rules on their own; (b, c) every public wrapper of hamming.py, driven by
the table of tests/wrapper_arg_cases.py, under a recording stand-in for the library -- no tensor form a caller can hand over
reaches an entry point as a raw pointer of the wrong layout or dtype, and no refused form reaches one at all; (d) the host
twins on real data: every accepted form gives the canonical call's result, which is the oracle's."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import ndcg_cases
import wrapper_arg_cases as C
from oracle import ranking
from wvhash import _lib
from wvhash.engine import CustomCalculator, _args
from wvhash.engine import hamming as H
from wvhash.engine import hamming_host as HH

AP_TOL = 1e-6                    # tests/test_gpu_ranking.py's: fp32 AP against the oracle's
CPU = torch.device("cpu")
to_meta = lambda t: t.to("meta")            # noqa: E731


# --------------------------------------------------------------------------------------------------- a. the gate on its own
def _g(t, dtype=torch.int64, shape=(None, None), kind=_args.ROWS, device=CPU):
    return _args.gate(t, "some_wrapper", "some_arg", dtype, device, shape, kind)


def test_gate_passes_a_canonical_tensor_untouched():
    x = torch.arange(12, dtype=torch.int64).view(6, 2)
    for kind in (_args.ROWS, _args.PITCH, _args.WRITTEN):
        got = _g(x, kind=kind)
        assert got is x and got.data_ptr() == x.data_ptr()
    lists = torch.zeros((6, 5), dtype=torch.int32)
    assert _g(lists, _args.INDEX, kind=_args.PITCH).data_ptr() == lists.data_ptr()


def test_gate_plain_rows_any_stride_or_offset_is_copied_when_not_contiguous():
    base = torch.arange(48, dtype=torch.int64).view(12, 4)
    for view in (base[::2], base[:, :2], base[:, 1:3], base.t().contiguous().t()):
        assert not view.is_contiguous()
        got = _g(view)
        assert got.is_contiguous() and torch.equal(got, view) and got.data_ptr() != view.data_ptr()
    tail = base[1:]                                            # a storage offset alone is canonical: kept
    assert _g(tail).data_ptr() == tail.data_ptr() and tail.storage_offset() == 4


def test_gate_row_pitch_is_kept_and_anything_else_copied():
    wide = torch.arange(60, dtype=torch.int32).view(6, 10)
    for kept in (wide[:, :4], wide[::2], wide[::2, :7]):      # stride(1) == 1, stride(0) >= shape[1]
        got = _g(kept, _args.INDEX, kind=_args.PITCH)
        assert got.data_ptr() == kept.data_ptr() and got.stride() == kept.stride()
    for copied in (wide[:, ::2], wide.t().contiguous().t(), wide[:1].expand(6, 10)):
        got = _g(copied, _args.INDEX, kind=_args.PITCH)
        assert got.is_contiguous() and torch.equal(got, copied) and got.data_ptr() != copied.data_ptr()
    cube = torch.zeros((2, 3, 4), dtype=torch.uint8)           # the pitch rule is 2-D: anything else is plain rows
    assert _g(cube[:, :, :2], torch.uint8, (None, None, None), _args.PITCH).is_contiguous()


def test_gate_dtype_only_index_lists_are_converted():
    lists = torch.arange(20, dtype=torch.int64).view(4, 5)
    got = _g(lists, _args.INDEX, kind=_args.PITCH)
    assert got.dtype == torch.int32 and torch.equal(got.long(), lists)
    got = _g(lists[:, :3], _args.INDEX)                       # converted and made contiguous
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got.long(), lists[:, :3])
    for bad in (torch.int16, torch.uint8, torch.float32, torch.float64):
        with pytest.raises(ValueError, match=r"some_wrapper: some_arg: expected dtype torch\.int32"):
            _g(lists.to(bad), _args.INDEX)
    with pytest.raises(ValueError, match="some_wrapper: some_arg"):            # a written index buffer is never converted
        _g(lists, _args.INDEX, kind=_args.WRITTEN)
    for declared, bad in ((torch.int64, torch.int32), (torch.int64, torch.float64), (torch.uint8, torch.int32),
                          (torch.int16, torch.int32), (torch.int32, torch.int64), (torch.int64, torch.complex128)):
        assert _g(torch.zeros((2, 2), dtype=declared), declared).dtype == declared
        with pytest.raises(ValueError, match="some_wrapper: some_arg: expected dtype"):
            _g(torch.zeros((2, 2), dtype=bad), declared)


def test_gate_written_buffers_are_never_copied():
    buf = torch.zeros((6, 4), dtype=torch.int64)
    assert _g(buf, kind=_args.WRITTEN) is buf
    assert _g(buf[2:], kind=_args.WRITTEN).data_ptr() == buf[2:].data_ptr()
    for bad in (buf[::2], buf[:, :2], buf.t()):
        with pytest.raises(ValueError, match="some_wrapper: some_arg: a buffer that is written must be contiguous"):
            _g(bad, shape=(None, None), kind=_args.WRITTEN)
    with pytest.raises(ValueError, match="some_wrapper: some_arg: expected dtype"):
        _g(buf.int(), kind=_args.WRITTEN)
    with pytest.raises(ValueError, match="some_wrapper: some_arg: expected shape"):
        _g(buf, shape=(5, 4), kind=_args.WRITTEN)


def test_gate_shape_agreement():
    x = torch.zeros((6, 2), dtype=torch.int64)
    assert _g(x, shape=(6, None)) is x and _g(x, shape=(None, 2)) is x and _g(x, shape=(6, 2)) is x
    for shape in ((3, None), (None, 1), (None,), (None, None, None), (6, 2, 1)):
        with pytest.raises(ValueError, match=r"some_wrapper: some_arg: expected shape \["):
            _g(x, shape=shape)
    with pytest.raises(ValueError, match="some_wrapper: some_arg: expected a tensor"):
        _g(np.zeros((6, 2), dtype=np.int64))


def test_gate_device_rule_on_meta_tensors():
    meta = torch.device("meta")
    x, m = torch.zeros((6, 2), dtype=torch.int64), torch.zeros((6, 2), dtype=torch.int64, device="meta")
    assert _g(m, device=meta) is m and _g(x, device=CPU) is x
    with pytest.raises(ValueError, match="some_wrapper: some_arg: lives on meta, expected cpu"):
        _g(m, device=CPU)
    with pytest.raises(ValueError, match="some_wrapper: some_arg: lives on cpu, expected meta"):
        _g(x, device=meta)
    assert _args.anchor(x, "w", "a", "cpu") == CPU and _args.anchor(m, "w", "a", "meta") == meta
    with pytest.raises(ValueError, match="w: a: expected a tensor on a cuda device"):
        _args.anchor(x, "w", "a", "cuda")


def test_the_table_covers_every_public_wrapper():
    named = {"bit_counts", "hamming_dist", "hamming_topk", "hamming_hist", "hamming_topk_rows16", "hamming_shard_prefix", "topk_merge",
             "topk_merge_cum", "rank_from_dist", "map_at_k", "map_at_ks", "hit_prefix", "label_overlap_hist", "ndcg_at_ks",
             "hamming_map_at_k", "hamming_map_at_ks", "hamming_radius_hist", "hamming_shard_relbits", "merge_relbits_map",
             "merge_relbits_map_ks", "PreparedDB", "PreparedLabels"}
    assert C.PUBLIC == named and all(hasattr(H, n) for n in named)
    assert {c.name for c in C.CASES if c.twin} == {n for n in named if hasattr(HH, n)} - {"hamming_map_at_k", "hamming_map_at_ks"}


# ------------------------------------------------------------------------- c. the GPU wrappers under a recording stand-in
class StandIn:
    """Stands where the library stands: every wv_* entry point records its name and arguments and answers 0 (a size query:
    64 bytes).  No kernel runs; outputs stay uninitialised."""

    def __init__(self):
        self.calls, self.tensors = [], []

    def __getattr__(self, name):
        if not name.startswith("wv_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 64 if name.endswith("_bytes") else 0
        return entry

    def entries(self):
        """entry points that were handed pointers (size queries take none)"""
        return [name for name, _ in self.calls if not name.endswith("_bytes")]

    def pointers(self):
        out = set()
        for _, args in self.calls:
            for a in args:
                if isinstance(a, ctypes.c_void_p):
                    out.add(a.value or 0)
                elif isinstance(a, int):
                    out.add(a)
        return out

    def clear(self):
        self.calls, self.tensors = [], []


@pytest.fixture
def standin(monkeypatch):
    """hamming.py on host tensors: the library loader, the stream getter and the device context replaced, _lib.ptr
    remembering what it is given; the module takes host tensors for its own kind and keeps no discount table."""
    lib = StandIn()
    real_ptr = _lib.ptr

    def ptr(t):
        if t is not None:
            lib.tensors.append(t)
        return real_ptr(t)
    monkeypatch.setattr(_lib, "require_gpu", lambda: lib)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(_lib, "ptr", ptr)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(H, "_DEVICE_TYPE", "cpu")
    monkeypatch.setattr(H, "_NDCG_WEIGHTS", {})
    return lib


def _conforms(t, arg):
    pitched = arg.kind == C.PITCH and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]
    return t.dtype == arg.declared and (t.is_contiguous() or pitched)


def _layout_ok(t):
    return t.is_contiguous() or (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1])


def _setup(run, Hm):
    case, cfg, k = run
    w = C.world(*cfg)
    a = {name: t.clone() for name, t in case.canon(w, k).items()}
    return case, w, k, a, case.prepare(Hm, a)


@pytest.mark.parametrize("run", C.runs(), ids=C.run_id)
def test_standin_accepted_forms_reach_the_library_in_the_declared_form(standin, run):
    case, w, k, a, x = _setup(run, H)
    want = case.want(w, k)
    for arg in case.args:
        for form in ["canonical"] + C.accepted_forms(arg):
            given = a[arg.name] if form == "canonical" else C.make_accepted(form, arg, a[arg.name])
            standin.clear()
            out = case.call(H, w, k, dict(a, **{arg.name: given}), x)
            what = (case.name, arg.name, form)
            assert standin.entries(), what
            assert all(_layout_ok(t) for t in standin.tensors), what
            if _conforms(given, arg):                          # kept as it is: no copy
                assert given.data_ptr() in standin.pointers(), what
            else:                                              # the raw pointer of what the caller passed never arrives
                assert given.data_ptr() not in standin.pointers(), what
            if arg.name != "wire":                             # (a wire buffer's pointers are _wire_args' integers, checked above)
                arrived = [t for t in standin.tensors if t.shape == given.shape and t.dtype == arg.declared
                           and torch.equal(t, a[arg.name].to(arg.declared))]
                assert arrived and all(_conforms(t, arg) for t in arrived), what
            assert len(out) == len(want), what
            for o, e in zip(out, want):
                assert (o is None) == (e is None), what
                if e is not None:
                    assert tuple(o.shape) == tuple(e[0].shape), what
                    assert o.dtype == (torch.float32 if e[1] == C.AP else e[0].dtype), what


@pytest.mark.parametrize("run", C.runs(), ids=C.run_id)
def test_standin_refused_forms_never_reach_an_entry_point(standin, run):
    case, w, k, a, x = _setup(run, H)
    for arg in case.args:
        for form in C.refused_forms(arg):
            given = C.make_refused(form, arg, a[arg.name], to_meta)
            standin.clear()
            with pytest.raises(ValueError, match=case.name.replace("_want_cum", "")):
                case.call(H, w, k, dict(a, **{arg.name: given}), x)
            assert standin.entries() == [], (case.name, arg.name, form, standin.entries())


def test_standin_the_gpu_module_takes_no_host_tensor(standin, monkeypatch):
    """Without the stand-in's change of the module's device kind, host tensors are refused before any entry point."""
    monkeypatch.setattr(H, "_DEVICE_TYPE", "cuda")
    w = C.world(*C.WORLDS[2])
    idx = w.order[:, :100].contiguous()
    for call in (lambda: H.hamming_topk(w.qp, w.rp, w.nbits, 100), lambda: H.map_at_k(idx, w.qlp, w.rlp), lambda: H.PreparedDB(w.rp),
                 lambda: H.bit_counts(w.rp, w.nbits), lambda: H.topk_merge(idx[None], w.order_d[None, :, :100], 100, w.nbits)):
        with pytest.raises(ValueError, match="expected a tensor on a cuda device"):
            call()
    assert standin.entries() == []


def test_standin_prepared_objects_of_another_device_are_refused(standin):
    w = C.world(*C.WORLDS[2])
    db, labels = H.PreparedDB(w.rp), H.PreparedLabels(w.rlp)
    standin.clear()
    db.packed = db.packed.to("meta")
    with pytest.raises(ValueError, match="hamming_topk: db: lives on meta"):
        H.hamming_topk(w.qp, db, w.nbits, 100)
    with pytest.raises(ValueError, match="hamming_map_at_k: db: lives on meta"):
        H.hamming_map_at_k(w.qp, db, labels, w.qlp, w.nbits, 100)
    assert standin.entries() == []


def test_standin_int64_lists_reach_map_at_k_as_int32(standin):
    """The headline case: get_knn hands out idx.long(); read as int32 pairs every second entry would be row 0."""
    w = C.world(*C.WORLDS[2])
    lists = w.order[:, :100].long()
    for call in (lambda: H.map_at_k(lists, w.qlp, w.rlp), lambda: H.map_at_ks(lists, w.qlp, w.rlp, C.KS),
                 lambda: H.hit_prefix(lists, w.qlp, w.rlp), lambda: H.ndcg_at_ks(lists, w.qlp, w.rlp, C.KS, hist=w.hist)):
        standin.clear()
        call()
        assert lists.data_ptr() not in standin.pointers()
        assert not any(t.dtype == torch.int64 and t.shape == lists.shape for t in standin.tensors)
        assert any(t.dtype == torch.int32 and t.shape == lists.shape and torch.equal(t.long(), lists) for t in standin.tensors)


# ------------------------------------------------------------------------------------------ d. the host twins on real data
def _assert_outputs(out, want, what, k):
    assert len(out) == len(want), what
    for o, e in zip(out, want):
        assert (o is None) == (e is None), what
        if e is None:
            continue
        exp, mode = e
        assert tuple(o.shape) == tuple(exp.shape), what
        if mode == C.EXACT:
            assert o.dtype == exp.dtype and torch.equal(o.cpu(), exp), what
        elif mode == C.AP:
            assert o.dtype == torch.float32 and float((o.cpu().double() - exp).abs().max()) <= AP_TOL, what
        elif mode == C.DCG:
            tol = torch.tensor([ndcg_cases.sum_tol(kk) for kk in C.KS], dtype=torch.float64)
            assert o.dtype == torch.float64 and bool(((o.cpu() - exp).abs() <= tol * exp.abs()).all()), what


def _same(out, canon, what):
    for o, c in zip(out, canon):
        assert (o is None and c is None) or (o.dtype == c.dtype and torch.equal(o, c)), what


@pytest.mark.parametrize("run", C.runs(twin_only=True), ids=C.run_id)
def test_host_twins_accept_every_form_and_refuse_the_rest(run):
    case, w, k, a, x = _setup(run, HH)
    canon = case.call(HH, w, k, a, x)
    _assert_outputs(canon, case.want(w, k), (case.name, "canonical"), k)
    for arg in case.args:
        for form in C.accepted_forms(arg):
            given = C.make_accepted(form, arg, a[arg.name])
            _same(case.call(HH, w, k, dict(a, **{arg.name: given}), x), canon, (case.name, arg.name, form))
        for form in C.refused_forms(arg):
            with pytest.raises(ValueError, match=case.name):
                case.call(HH, w, k, dict(a, **{arg.name: C.make_refused(form, arg, a[arg.name], to_meta)}), x)


def test_host_int64_lists_give_the_ap_of_int32_lists_and_the_oracle():
    """map_at_k(hamming_topk(...)[0].long(), ...) on the host twin, and CustomCalculator(device='cpu') around it."""
    w = C.world(*C.WORLDS[0])
    k = 100
    idx = HH.hamming_topk(w.qp, w.rp, w.nbits, k)[0]
    assert torch.equal(idx, w.order[:, :k])
    ap32, nrel32 = HH.map_at_k(idx, w.qlp, w.rlp)
    ap64, nrel64 = HH.map_at_k(idx.long(), w.qlp, w.rlp)
    assert torch.equal(ap64, ap32) and torch.equal(nrel64, nrel32)
    assert float((ap64.double() - w.ap(k)[0]).abs().max()) <= AP_TOL and torch.equal(nrel64, w.ap(k)[1])
    assert float(nrel64.max()) > 0
    calc = CustomCalculator(k=k, device="cpu", distance_metric="hamming", with_faiss=False)
    want = ranking.calculate_maphashing(w.q, w.ql, w.r, w.rl, k, stable=True)
    assert abs(calc.calculate_maphashing(w.q, w.ql, w.r, w.rl, k) - want) < AP_TOL
    assert abs(float(ap64.double().mean()) - want) < AP_TOL


def test_host_short_label_rows_are_refused_not_read_past():
    """3 label rows for 6 lists: refused by the gate on the host twin too."""
    w = C.world(*C.WORLDS[2])
    idx = w.order[:6, :100].contiguous()
    for fn in (HH.map_at_k, HH.hit_prefix):
        with pytest.raises(ValueError, match=r"qlab_packed: expected shape \[6, \*\]"):
            fn(idx, w.qlp[:3], w.rlp)
