"""wvhash/models/_prepared.py: the one cache of what the eval-mode wrappers derive from their parameters.  Host only."""
import copy
import threading
import time

import torch
import torch.nn as nn

from wvhash.models import get_fusion_head
from wvhash.models._prepared import PreparedCache, param_key
from wvhash.models.dsln import MultiDomainLayerNorm


def test_param_key_follows_storage_and_version():
    a, b = torch.zeros(3), torch.zeros(3)
    key = param_key(a, b)
    assert key == ((a.data_ptr(), a._version), (b.data_ptr(), b._version)) and param_key(a, b) == key
    a.add_(1)
    assert param_key(a, b) != key and param_key(a, b)[1] == key[1]
    assert param_key(a.clone(), b)[0] != param_key(a, b)[0]


def test_hit_miss_peek_and_devices_side_by_side():
    cache, built = PreparedCache(), []

    def build(tag):
        def make():
            built.append(tag)
            return [tag]
        return make
    assert cache.peek("fp32", "cuda:0") is None
    v0 = cache.get("fp32", "cuda:0", ("k", 0), build("a"))
    assert v0 == ["a"] and cache.peek("fp32", "cuda:0") == (("k", 0), ["a"]) and cache.peek("fp32", "cuda:0")[1] is v0
    assert cache.get("fp32", "cuda:0", ("k", 0), build("never")) is v0 and built == ["a"]             # hit: the same object
    v1 = cache.get("fp32", "cuda:1", ("k", 0), build("b"))                                            # same key, other device
    assert v1 == ["b"] and cache.get("fp32", "cuda:0", ("k", 0), build("never")) is v0
    assert cache.peek("fp32", "cuda:0")[1] is v0 and cache.peek("fp32", "cuda:1")[1] is v1
    v2 = cache.get("bf16", "cuda:0", ("k", 0), build("c"))                                            # other slot, same device
    assert v2 == ["c"] and cache.peek("fp32", "cuda:0")[1] is v0 and cache.peek("bf16", "cuda:1") is None
    v3 = cache.get("fp32", "cuda:0", ("k", 1), build("d"))                                            # miss: replaced whole
    assert v3 == ["d"] and cache.peek("fp32", "cuda:0") == (("k", 1), ["d"]) and cache.peek("fp32", "cuda:1")[1] is v1
    assert built == ["a", "b", "c", "d"]
    assert cache.get("fp32", torch.device("cpu"), 0, build("e")) == ["e"] and cache.peek("fp32", torch.device("cpu"))[1] == ["e"]
    assert not hasattr(cache, "clear")


def test_concurrent_readers_get_what_their_key_built():
    """Replicas call from concurrent threads: every value returned was built from the key it was asked with, on the device
    it was asked for, whatever the other threads replace meanwhile."""
    cache, devices = PreparedCache(), ("cuda:0", "cuda:1", "cuda:2")
    THREADS, CALLS = 4, 1500
    errors, done = [], []

    def worker(t):
        try:
            for i in range(CALLS):
                dev, key = devices[(i + t) % len(devices)], ("params", (i + 7 * t) // 50)

                def build(dev=dev, key=key):
                    time.sleep(0)                       # yields the GIL between the miss and the store
                    return (dev, key)
                value = cache.get("fp32", dev, key, build)
                if value != (dev, key):
                    errors.append((t, i, dev, key, value))
                seen = cache.peek("fp32", dev)
                if seen is None or seen[1] != (dev, seen[0]):
                    errors.append((t, i, dev, "peek", seen))
            done.append(t)
        except Exception as e:                          # noqa: BLE001  reported below, in the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
        assert not th.is_alive(), "a worker did not finish"
    assert not errors, errors[:5]
    assert sorted(done) == list(range(THREADS))


def test_replicas_share_the_cache():
    head = get_fusion_head({"type": "cross_attention_advanced", "output_dim": 64, "num_queries": 4, "num_heads": 4}, [64] * 4)
    norm = MultiDomainLayerNorm(nn.LayerNorm(32), num_domains=4)
    for module in (head, norm):
        assert isinstance(module._prepared, PreparedCache)
        assert copy.copy(module)._prepared is module._prepared
        assert module._replicate_for_data_parallel()._prepared is module._prepared
    assert head._prepared is not norm._prepared


def test_group_layernorm_affine_is_cached_per_parameter_state():
    norm = MultiDomainLayerNorm(nn.LayerNorm(32), num_domains=4)
    cpu = torch.device("cpu")
    gamma, beta = norm._affine(cpu)
    assert tuple(gamma.shape) == tuple(beta.shape) == (4, 32) and norm._affine(cpu)[0] is gamma
    assert copy.copy(norm)._affine(cpu)[0] is gamma                     # a replica reads what the module built
    with torch.no_grad():
        norm.norms[2].weight.mul_(2.0)
    gamma2, _ = norm._affine(cpu)
    assert gamma2 is not gamma and torch.equal(gamma2[2], norm.norms[2].weight) and torch.equal(gamma2[0], gamma[0])
