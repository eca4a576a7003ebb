"""What the benchmark tools of the fused losses and of the batch mAP proxy share: the clock, the spread of a list of times, the
memory peak of one call, and the fused-against-plain measurement of one loss at one shape."""
import statistics

import torch


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def fused_against_plain(fused, plain, warmup, rounds, calls, memory=False):
    """fused, plain: one step of either path, () -> (value, gradient).  Their numbers are compared first (value relative,
    gradient norm-wise); then, after `warmup` calls of both, the variants alternate inside every round: median [min, max]
    over rounds x calls single calls, HIP events around the call.  memory: also the peak of
    torch.cuda.max_memory_allocated over one call of each, above what was allocated before it.  -> the JSON keys of one
    loss at one shape."""
    variants = {"fused": fused, "plain": plain}
    (fv, fg), (pv, pg) = fused(), plain()
    out = {"value_rel_diff": abs(float(fv) - float(pv)) / abs(float(pv)),
           "grad_normwise_diff": float((fg - pg).abs().max() / pg.abs().max()), "calls_per_variant": rounds * calls}
    for _ in range(warmup):                                                  # code objects, allocator, clocks
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    mem = {v: peak_bytes(fn) for v, fn in variants.items()} if memory else {}
    ms = {v: [] for v in variants}
    for _ in range(rounds):                                                  # alternating
        for v, fn in variants.items():
            ms[v] += [event_ms(fn) for _ in range(calls)]
    med = {v: statistics.median(t) for v, t in ms.items()}
    out.update({v: spread(t) for v, t in ms.items()})
    out.update({f"{v}_peak_bytes": b for v, b in mem.items()})
    out.update(plain_over_fused=round(med["plain"] / med["fused"], 3), fused_faster_than_plain=bool(med["fused"] < med["plain"]))
    return out
