"""What an eval-mode wrapper derives from its parameters alone (projected queries, re-laid-out weights, stacked affine
rows) and keeps between calls: one cache shape and one key formula for every module that does so.

A module's replicas (``copy.copy``, ``nn.Module._replicate_for_data_parallel``) share the cache object, and nn.DataParallel
runs them from concurrent threads.  Each (slot, device) holds one ``(key, value)`` pair that is only ever replaced whole, by
one item assignment: a reader gets the old pair or the new one, never a mixture, and never what another device built.
"""


def param_key(*tensors):
    """Identity of the tensors something was derived from: storage pointer and version counter of each (an in-place
    update bumps the version, a move or a reload changes the pointer)."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


class PreparedCache:
    def __init__(self):
        self._entries = {}          # (slot, device) -> (key, value)

    def get(self, slot, device, key, build):
        """The value stored for (slot, device) if it was built from `key`, else `build()`, which replaces it."""
        entry = self._entries.get((slot, device))
        if entry is None or entry[0] != key:
            entry = (key, build())
            self._entries[(slot, device)] = entry
        return entry[1]

    def peek(self, slot, device):
        """(key, value) of (slot, device), or None: for tests and tools."""
        return self._entries.get((slot, device))
