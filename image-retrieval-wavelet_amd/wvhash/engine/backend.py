"""Where the ranking stage runs: the one place that reads a `device` argument.

A backend is the primitives module (engine/hamming.py on the GPU, its name-for-name host mirror engine/hamming_host.py), the
move of a tensor (or anything torch.as_tensor takes) to that side, and the real-valued k-NN.  The host is explicit, never a
fallback: device=None / 'cuda' is the GPU backend, whose first call raises WvhashUnavailable on a machine without one.
Callers reach the primitives through the module attribute (B.H.hamming_topk(...)): nothing is bound here.
"""
from collections import namedtuple

import torch

from . import hamming, hamming_host
from .get_knn import _to_gpu, knn_float, knn_float_host

Backend = namedtuple("Backend", "H move knn_float")


def _to_host(x):
    return (x if torch.is_tensor(x) else torch.as_tensor(x)).detach().cpu()


GPU = Backend(hamming, _to_gpu, knn_float)
HOST = Backend(hamming_host, _to_host, knn_float_host)


def backend(device=None):
    """None, 'cuda', 'cpu' or a torch.device -> GPU or HOST."""
    return HOST if device is not None and torch.device(device).type == "cpu" else GPU
