"""Shared by tests/test_hash_tail_cases.py (no GPU) and tests/test_gpu_hash_tail.py: the dispatch rule of wv_hash_tail
(csrc/head.hip) restated in plain Python, the sweep of (E, nbits, B) points with the kernel each pin must reach there,
seeded random and exactly representable inputs, the float64 reference with its derived per-element bound, and one caller
of wv_hash_tail / wv_hash_tail_cpu through ctypes that pre-fills every output and guards it with a sentinel tail.

The three kernels: "simple" (k_hash_tail, one fmaf chain per logit), "valu16" (k_hash_tail16, the same chain for 16
samples per workgroup) and "mfma" (k_hash_tail_mfma, four k ranges on the matrix cores summed in a fixed order).
"""
import functools

import numpy as np

KERNELS = ("simple", "valu16", "mfma")
PINS = (None, "simple", "valu16", "mfma")              # WV_HASH_TAIL of the diagnostic library; None = unset
SETS = ("plain", "bias", "bn", "bias_bn")              # hash_fc bias / BatchNorm1d present
MAX_LDS = 160 * 1024                                   # kMaxLdsBytes
WV_OK, WV_EINVAL = 0, -22


def route(B, E, pin):
    """The kernel wv_hash_tail launches for a batch of B samples of width E under the pin."""
    if pin not in ("simple", "valu16") and E % 32 == 0 and (B >= 32 or pin == "mfma"):
        return "mfma"
    if 324 * E <= MAX_LDS - 1024 and B >= 64 and pin != "simple":
        return "valu16"
    return "simple"


# ------------------------------------------------------------------------------------------------ the sweep
# (E, nbits, B) -> the kernels the pins (None, simple, valu16, mfma) reach, one letter each; written by hand, held against
# route() by every test that uses a point, so that a change of the rule moves no case to another kernel unnoticed.
ES = (4, 8, 32, 100, 384, 416, 500, 504, 768, 1024)
NBITS = (1, 31, 32, 33, 63, 64, 65, 96, 128, 250, 257)
BS = (1, 31, 32, 33, 63, 64, 65, 100)
_E_SWEEP = {4: "VSVV", 8: "VSVV", 32: "MSVM", 100: "VSVV", 384: "MSVM", 416: "MSVM", 500: "VSVV", 504: "SSSS", 768: "MSSM",
            1024: "MSSM"}                                                    # nbits = 96, B = 65
_B_SWEEP = {1: "SSSM", 31: "SSSM", 32: "MSSM", 33: "MSSM", 63: "MSSM", 64: "MSVM", 65: "MSVM", 100: "MSVM"}   # E = 384, nbits = 32
LETTER = {"S": "simple", "V": "valu16", "M": "mfma"}


def _points():
    pts = {}
    for E in ES:
        pts[(E, 96, 65)] = _E_SWEEP[E]
    for n in NBITS:
        pts[(64, n, 33)] = "MSSM"
        pts[(384, n, 65)] = "MSVM"
    for B in BS:
        pts[(384, 32, B)] = _B_SWEEP[B]
    return pts


POINTS = _points()                                     # insertion-ordered; a point two sweeps share appears once
# one run per point and pin: (E, nbits, B, pin, parameter set, expected kernel); the four sets rotate over points and pins
RUNS = [(E, n, B, pin, SETS[(i + p) % 4], LETTER[letters[p]])
        for i, ((E, n, B), letters) in enumerate(POINTS.items()) for p, pin in enumerate(PINS)]


def run_id(run):
    E, n, B, pin, pset, kern = run
    return f"E{E}-n{n}-B{B}-{pin or 'auto'}-{pset}-{kern}"


# ------------------------------------------------------------------------------------------------ inputs
def _seed(E, nbits, B, pset):
    return 100003 * E + 1009 * nbits + 17 * B + SETS.index(pset)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_case(E, nbits, B, pset):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(E); BatchNorm with running_var in [0.5, 2], eps = 1e-5, weights of both signs and (from
    two bits on) one channel of weight exactly 0, bias and running_mean ~ 0.1 N(0, 1)."""
    g = np.random.default_rng(_seed(E, nbits, B, pset))
    c = {"E": E, "nbits": nbits, "B": B, "pset": pset, "kind": "random", "eps": 0.0,
         "x": _f32(g.standard_normal((B, E))), "w": _f32(g.standard_normal((nbits, E)) / np.sqrt(E)),
         "hb": None, "bn_w": None, "bn_b": None, "bn_mean": None, "bn_var": None}
    if pset in ("bias", "bias_bn"):
        c["hb"] = _f32(0.1 * g.standard_normal(nbits))
    if pset in ("bn", "bias_bn"):
        gamma = g.standard_normal(nbits)
        if nbits > 1:
            gamma[nbits // 2] = 0.0
        c.update(bn_w=_f32(gamma), bn_b=_f32(0.1 * g.standard_normal(nbits)), bn_mean=_f32(0.1 * g.standard_normal(nbits)),
                 bn_var=_f32(g.uniform(0.5, 2.0, nbits)), eps=1e-5)
    return c


@functools.lru_cache(maxsize=None)
def exact_case(E, nbits, B, pset, nonfinite=True):
    """Integers in [-3, 3] for x and w (every product and partial sum is exact in fp32 in any order: 9 * 1024 < 2^24), an integer
    bias; BatchNorm with eps = 0, running_var in {0.25, 1, 4, 16}, weights +-{0.5, 1, 2}, integer running_mean and bias: every
    operation of the expression is exact.  Column 0 has bias = running_mean = bn bias = 0; from 4 bits on row 1 of w is zero
    (with the same neutral parameters: logit exactly 0 for every finite sample) and w[3] = -w[2]; from 4 samples on sample 0
    is all zero.  nonfinite: sample B - 1 holds a NaN and sample B - 2 a +inf (B >= 3); without it the two rows keep their integers."""
    g = np.random.default_rng(_seed(E, nbits, B, pset) + 7)
    x = g.integers(-3, 4, (B, E)).astype(np.float32)
    w = g.integers(-3, 4, (nbits, E)).astype(np.float32)
    neutral = [0]
    if nbits >= 4:
        w[1] = 0.0
        w[3] = -w[2]
        neutral.append(1)
    if B >= 4:
        x[0] = 0.0
    if nonfinite and B >= 3:
        x[B - 1, E // 3] = np.nan
        x[B - 2, E // 2] = np.inf
    c = {"E": E, "nbits": nbits, "B": B, "pset": pset, "kind": "exact", "eps": 0.0, "x": _f32(x), "w": _f32(w),
         "hb": None, "bn_w": None, "bn_b": None, "bn_mean": None, "bn_var": None,
         "nan_row": B - 1 if nonfinite and B >= 3 else None, "inf_row": B - 2 if nonfinite and B >= 3 else None}
    if pset in ("bias", "bias_bn"):
        hb = g.integers(-5, 6, nbits).astype(np.float32)
        hb[neutral] = 0.0
        c["hb"] = _f32(hb)
    if pset in ("bn", "bias_bn"):
        gamma = g.choice([0.5, 1.0, 2.0], nbits) * g.choice([-1.0, 1.0], nbits)
        beta, mean = g.integers(-4, 5, nbits).astype(np.float64), g.integers(-4, 5, nbits).astype(np.float64)
        beta[neutral], mean[neutral] = 0.0, 0.0
        c.update(bn_w=_f32(gamma), bn_b=_f32(beta), bn_mean=_f32(mean), bn_var=_f32(g.choice([0.25, 1.0, 4.0, 16.0], nbits)))
    return c


def rows(case, lo, hi):
    """The same case with samples lo .. hi - 1 only."""
    c = dict(case)
    c["x"], c["B"] = _f32(case["x"][lo:hi]), hi - lo
    return c


# ------------------------------------------------------------------------------------------------ reference
def reference(case):
    """-> (float64 logits [B, nbits], per-element bound tol).  logits = x64 @ w64.T + hb, then BatchNorm with np.sqrt, all in
    float64.  tol = (E + 8) 2^-24 ((sum_k |x_k| |w_k| + |hb| + |mean|) |gamma| / sqrt(var + eps) + |beta|): the forward
    bound of an E-term fp32 (fused) chain plus a few roundings for bias, BatchNorm and the four-way partial sums of the
    matrix-core kernel.  It holds for any summation order: one bound for the three kernels and the host twin."""
    x, w = case["x"].astype(np.float64), case["w"].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        odd = np.flatnonzero(~np.isfinite(x).all(axis=1))          # rows with a NaN or an infinity: product by product, not BLAS
        xf = x.copy()
        xf[odd] = 0.0
        ref = xf @ w.T
        ref[odd] = (x[odd][:, None, :] * w[None, :, :]).sum(axis=2)
        mag = np.abs(x) @ np.abs(w).T
        if case["hb"] is not None:
            ref = ref + case["hb"].astype(np.float64)
            mag = mag + np.abs(case["hb"].astype(np.float64))
        scale, beta = 1.0, 0.0
        if case["bn_w"] is not None:
            gamma, mean = case["bn_w"].astype(np.float64), case["bn_mean"].astype(np.float64)
            sd = np.sqrt(case["bn_var"].astype(np.float64) + np.float64(np.float32(case["eps"])))
            beta = case["bn_b"].astype(np.float64)
            ref = (ref - mean) / sd * gamma + beta
            mag, scale = mag + np.abs(mean), np.abs(gamma) / sd
        tol = (case["E"] + 8) * 2.0 ** -24 * (mag * scale + np.abs(beta))
    return ref, tol


def left_out(case):
    """Fraction of the elements whose reference is too close to zero for the sign check (|ref| <= tol)."""
    ref, tol = reference(case)
    return float(np.mean(np.abs(ref) <= tol))


# ------------------------------------------------------------------------------------------------ the call
NAN_FILL = 0x7FC5A5A5                                  # a quiet NaN no arithmetic produces (payload), as int32
PACK_FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
TAIL_WORD, TAIL_PACK = 0x0BADF00D, np.uint64(0x0123456789ABCDEF)
TAIL_BYTES = 4096
OUTPUTS = ("logits", "codes", "packed")


def prefilled(B, nbits):
    """Host images of the three output buffers: the output region pre-filled (NaN / 0xA5 bytes), then a sentinel tail."""
    words, nt = (nbits + 63) // 64, TAIL_BYTES // 4
    fl = np.concatenate([np.full(B * nbits, NAN_FILL, np.int32), np.full(nt, TAIL_WORD, np.int32)])
    pk = np.concatenate([np.full(B * words, PACK_FILL, np.uint64), np.full(nt // 2, TAIL_PACK, np.uint64)])
    return {"logits": fl, "codes": fl.copy(), "packed": pk}


def call(case, where, want=OUTPUTS, B=None):
    """wv_hash_tail (where = "gpu", on the current stream of the current device) or wv_hash_tail_cpu ("cpu") through ctypes
    with the outputs named in `want`, the others NULL.  -> (rc, {name: whole buffer as numpy, tail included})."""
    from wvhash import _lib
    lib = _lib.load()
    B = case["B"] if B is None else B
    bufs = {k: v for k, v in prefilled(B, case["nbits"]).items() if k in want}
    names = ("x", "w", "hb", "bn_w", "bn_b", "bn_mean", "bn_var")
    if where == "gpu":
        import torch
        dev = {k: torch.from_numpy(v.view(np.int64) if k == "packed" else v).cuda() for k, v in bufs.items()}
        ins = {k: torch.from_numpy(case[k].copy()).cuda() if case[k] is not None else None for k in names}
        p = {k: (t.data_ptr() if t is not None else None) for k, t in {**dev, **ins}.items()}
    else:
        p = {k: bufs[k].ctypes.data for k in bufs}
        p.update({k: (case[k].ctypes.data if case[k] is not None else None) for k in names})
    args = [p["x"], B, case["E"], p["w"], p["hb"], p["bn_w"], p["bn_b"], p["bn_mean"], p["bn_var"], float(case["eps"]),
            case["nbits"], p.get("logits"), p.get("codes"), p.get("packed")]
    if where == "gpu":
        rc = lib.wv_hash_tail(*args, _lib.stream_ptr())
        torch.cuda.synchronize()
        bufs = {k: t.cpu().numpy().view(bufs[k].dtype) for k, t in dev.items()}
    else:
        rc = lib.wv_hash_tail_cpu(*args)
    return rc, bufs


def outputs(case, bufs):
    """Checks the sentinel tails and that no pre-fill value is left; -> {name: the output region, shaped}."""
    B, nbits = case["B"], case["nbits"]
    words, out = (nbits + 63) // 64, {}
    for k, buf in bufs.items():
        n = B * (words if k == "packed" else nbits)
        tail, fill = (TAIL_PACK, PACK_FILL) if k == "packed" else (TAIL_WORD, NAN_FILL)
        assert buf.size - n >= TAIL_BYTES // buf.itemsize and np.all(buf[n:] == tail), f"{k}: written past its end"
        body = buf[:n]
        if k == "packed":
            assert not np.any(body.view(np.uint32) == np.uint32(0xA5A5A5A5)), "packed: a half-word nobody wrote"
            out[k] = body.reshape(B, words)
        else:
            left = np.flatnonzero(body == NAN_FILL)
            assert left.size == 0, f"{k}: {left.size} elements nobody wrote, first at (b, j) = {divmod(int(left[0]), nbits)}"
            out[k] = body.view(np.float32).reshape(B, nbits)
    return out


def run(case, where, want=OUTPUTS):
    rc, bufs = call(case, where, want)
    assert rc == WV_OK, rc
    return outputs(case, bufs)


def bits_of(packed, nbits):
    """uint64 [B, words] -> (bool [B, nbits], the pad bits [B, 64 words - nbits])."""
    B, words = packed.shape
    bits = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8).reshape(B, words * 8), axis=1, bitorder="little")
    return bits[:, :nbits].astype(bool), bits[:, nbits:]


def check_consistent(case, out):
    """What holds everywhere, whatever the rounding: codes = sign(own logits) with 0.0 for a zero and NaN passed through, the
    packed bit is own logit > 0, the pad bits of the last word are 0."""
    lg = out["logits"]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out["codes"], np.sign(lg), equal_nan=True)
        assert not np.any(np.signbit(out["codes"]) & (out["codes"] == 0)), "sign of a zero logit must be +0.0"
        bits, pad = bits_of(out["packed"], case["nbits"])
        assert not pad.any(), "pad bits above nbits must be 0"
        assert np.array_equal(bits, lg > 0)


def same_bits(a, b):
    """Two output dicts (or rows of them) equal bit for bit."""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def check_random(case, out):
    """-> max(err / tol).  Logits within the bound of the float64 reference; codes and bits decided by the reference wherever
    it is further than the bound from zero."""
    ref, tol = reference(case)
    ratio = np.abs(out["logits"].astype(np.float64) - ref) / tol
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[worst] <= 1.0, f"logit {worst}: {out['logits'][worst]!r} vs {ref[worst]!r}, {ratio[worst]:.3f} tol"
    sure = np.abs(ref) > tol
    assert np.array_equal(out["codes"][sure], np.sign(ref)[sure])
    assert np.array_equal(bits_of(out["packed"], case["nbits"])[0][sure], (ref > 0)[sure])
    check_consistent(case, out)
    return float(ratio.max())


def check_exact(case, out):
    """Logits equal the (exactly representable) float64 reference bit for bit: NaN where it is NaN, the same infinity where it
    is one.  Zero logits give code 0.0 and bit 0; a NaN row is NaN in logits and codes with all bits 0."""
    ref, _ = reference(case)
    lg = out["logits"]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(lg), nan), "NaN in other places than IEEE puts it"
    bad = np.argwhere(~nan & (lg.astype(np.float64) != ref))
    assert bad.size == 0, f"{len(bad)} logits differ from the exact value, first (b, j) = {tuple(bad[0])}: " \
                          f"{lg[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}"
    check_consistent(case, out)
    bits = bits_of(out["packed"], case["nbits"])[0]
    zero = ref == 0
    assert np.all(out["codes"][zero] == 0) and not bits[zero].any()
    assert np.all(np.isnan(out["codes"][nan])) and not bits[nan].any()
    if case["nan_row"] is not None:
        assert nan[case["nan_row"]].all()
        r = case["inf_row"]
        assert np.all(np.isinf(ref[r]) | nan[r])                   # inf times a zero weight is NaN, anything else +-inf
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out["codes"][r], np.sign(ref[r]), equal_nan=True)
