"""ctypes binding of libwvhash.so (C ABI: include/wvhash.h).

The product path has no CPU fallback: if the library is missing or fails to load, every op
raises ``WvhashUnavailable`` -- it never silently computes on the host.
"""
import contextlib
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# WVHASH_LIB: another build of the same library (A/B measurements of kernel variants, tools/build_variant.sh)
LIB_PATH = os.environ.get("WVHASH_LIB") or os.path.join(_HERE, "_lib", "libwvhash.so")
# The same objects linked with csrc/tune_diag.cpp: kernel-selection switches (WV_SWT_PATH, WV_HEAD_FRONT, WV_TOPK_V2, ...) are
# read from the environment.  The release library has them compiled out; only tests and tools/ load this one (diagnostic()).
DIAG_LIB_PATH = os.path.join(_HERE, "_lib", "libwvhash_diag.so")

WV_DT_U8, WV_DT_F32, WV_DT_BF16 = 0, 1, 2
WV_LAYOUT_NCHW, WV_LAYOUT_NHWC = 0, 1
WV_METRIC_IP, WV_METRIC_L2, WV_METRIC_L2_SQUARED = 0, 1, 2
WV_RANK_DESCENDING, WV_RANK_SQRT = 1, 2
ABI_VERSION = 5        # what include/wvhash.h documents; load() refuses a library that reports another one
WV_BANDS_INNER, WV_BANDS_OUTER = 0, 1
WV_TOKENS_SBE, WV_TOKENS_BSE = 0, 1      # band tokens as [S][B][E] (wv_band_attn_pool's) or [B][S][E] (torch.stack(kv_list, 1))
WV_RESAMPLE_BILINEAR, WV_RESAMPLE_BICUBIC = 2, 3      # PIL's enum values
WV_COLOUR_BRIGHTNESS, WV_COLOUR_CONTRAST, WV_COLOUR_SATURATION = 0, 1, 2
WV_IP_MAP_ROWS_MAX = 2048   # include/wvhash.h: rows wv_ip_map_at_k ranks in one workgroup
WV_PAIR_LOSS_SCH, WV_PAIR_LOSS_HASHNET = 0, 1
WV_PAIR_LOSS_ROWS_MAX = 2048   # include/wvhash.h: rows of a batch wv_pair_loss takes (D <= 512)
WV_RANK_AP_SMOOTH, WV_RANK_AP_SUP = 0, 1
WV_RANK_AP_QUICK, WV_RANK_AP_GENERAL = 0, 1
WV_RANK_AP_COLS_MAX = 4096     # include/wvhash.h: rows and columns of a score matrix wv_rank_ap takes
WV_ENOTSUP = -95           # return code: the shape is outside the kernel asked for (callers fall back)


class WvhashUnavailable(RuntimeError):
    pass


class WvhashError(RuntimeError):
    pass


class WvhashUnsupported(WvhashError):
    """WV_ENOTSUP from an entry point whose caller has another way to the same result."""


class HeadParams(ctypes.Structure):
    _fields_ = [
        ("embed_dim", ctypes.c_int), ("num_heads", ctypes.c_int), ("num_queries", ctypes.c_int),
        ("num_tokens", ctypes.c_int), ("pool_mean", ctypes.c_int),
        ("q_eff", ctypes.c_void_p), ("in_proj_w", ctypes.c_void_p), ("in_proj_b", ctypes.c_void_p),
        ("attn_out_w", ctypes.c_void_p), ("attn_out_b", ctypes.c_void_p),
        ("norm1_w", ctypes.c_void_p), ("norm1_b", ctypes.c_void_p),
        ("mlp0_w", ctypes.c_void_p), ("mlp0_b", ctypes.c_void_p),
        ("mlp2_w", ctypes.c_void_p), ("mlp2_b", ctypes.c_void_p),
        ("out_w", ctypes.c_void_p), ("out_b", ctypes.c_void_p),
        ("norm2_w", ctypes.c_void_p), ("norm2_b", ctypes.c_void_p),
        ("ln_eps", ctypes.c_float),
        ("q_proj", ctypes.c_void_p),
        ("prepared", ctypes.c_void_p),
    ]


class SizeStage(ctypes.Structure):
    """wv_size_stage: one step (crop -> resample -> window -> mirror) of one image; 80 bytes = 20 int32 words."""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64)] + [
        (name, ctypes.c_int32) for name in (
            "src_h", "src_w", "src_row_bytes", "crop_y", "crop_x", "crop_h", "crop_w", "res_h", "res_w",
            "win_y", "win_x", "out_h", "out_w", "dst_row_bytes", "filter", "flip")]


class ColourOps(ctypes.Structure):
    """wv_colour_ops: the colour operations of one image, in the order they run; 48 bytes = 12 32-bit words."""
    _fields_ = [("offset", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("row_bytes", ctypes.c_int32),
                ("n_ops", ctypes.c_int32), ("kind", ctypes.c_int32 * 3), ("factor", ctypes.c_float * 3)]


class PairLossParams(ctypes.Structure):
    """wv_pair_loss_params: which pairwise loss (WV_PAIR_LOSS_*) and its constants; 24 bytes."""
    _fields_ = [("kind", ctypes.c_int), ("apply_tanh", ctypes.c_int), ("pre_scale", ctypes.c_float),
                ("nbits", ctypes.c_float), ("alpha", ctypes.c_float), ("beta", ctypes.c_float)]


class RankApParams(ctypes.Structure):
    """wv_rank_ap_params: which rank approximation (WV_RANK_AP_SMOOTH | _SUP), which form (_QUICK | _GENERAL) and the
    constants; 28 bytes."""
    _fields_ = [("kind", ctypes.c_int), ("form", ctypes.c_int), ("tau", ctypes.c_float), ("rho", ctypes.c_float),
                ("offset", ctypes.c_float), ("delta", ctypes.c_float), ("start", ctypes.c_float)]


_vp, _i, _i64, _sz, _f =ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
_fp = ctypes.POINTER(ctypes.c_float)

# name -> (restype, argtypes); must list every symbol include/wvhash.h declares
SIGNATURES = {
    "wv_last_error": (ctypes.c_char_p, []),
    "wv_abi_version": (_i, []),
    "wv_swt2d_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "wv_swt2d_forward": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _fp, _fp, _i, _vp, _sz, _vp]),
    "wv_swt2d_forward_ex": (_i, [_vp, _i, _i, _vp, _i, _i, _i64, _i, _i, _i, _i, _i, _fp, _fp, _i, _vp, _sz, _vp]),
    "wv_swt2d_band_forward": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _i, _vp]),
    "wv_rawstack_forward": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "wv_swt2d_forward_cpu": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _fp, _fp, _i]),
    "wv_swt2d_band_forward_cpu": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _fp, _fp, _i]),
    "wv_rawstack_forward_cpu": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i]),
    "wv_dwt2d_forward_cpu": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _fp, _fp, _i]),
    "wv_pack_bits_cpu": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp]),
    "wv_bit_counts_cpu": (_i, [_vp, _i64, _i, _vp]),
    "wv_hamming_dist_cpu": (_i, [_vp, _vp, _vp, _i64, _i, _i64, _i]),
    "wv_hamming_topk_cpu": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i64]),
    "wv_map_at_k_cpu": (_i, [_vp, _i64, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "wv_hit_prefix_cpu": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp]),
    "wv_dwt_out_len": (_i, [_i, _i, _i]),
    "wv_dwt2d_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "wv_dwt2d_forward": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _fp, _fp, _i, _vp, _sz, _vp]),
    "wv_lifting2d_workspace_bytes": (_sz, [_i64, _i, _i]),
    "wv_lifting2d_forward": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "wv_pack_bits": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp, _vp]),
    "wv_bit_counts": (_i, [_vp, _i64, _i, _vp, _vp]),
    "wv_hamming_dist": (_i, [_vp, _vp, _vp, _i64, _i, _i64, _i, _vp]),
    "wv_hamming_topk_workspace_bytes": (_sz, [_i, _i64, _i, _i]),
    "wv_hamming_topk": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i64, _vp, _sz, _vp]),
    "wv_db_prepared_bytes": (_sz, [_i64, _i]),
    "wv_db_prepare": (_i, [_vp, _i64, _i, _vp, _sz, _vp]),
    "wv_hamming_dist_prepared": (_i, [_vp, _vp, _vp, _i64, _i, _i64, _i, _vp]),
    "wv_hamming_topk_prepared": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i64, _vp]),
    "wv_hamming_topk_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i64, _vp, _sz, _vp]),
    "wv_rank_labels_prepared_bytes": (_sz, [ctypes.c_int64, _i]),
    "wv_rank_labels_prepare": (_i, [_vp, ctypes.c_int64, _i, _vp, _sz, _vp]),
    "wv_hamming_map_at_k": (_i, [_vp, _vp, _vp, _vp, _i, _i, ctypes.c_int64, _i, _i, _vp, _vp, _vp]),
    "wv_hamming_radius_hist": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp]),
    "wv_hamming_radius_hist_cpu": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp]),
    "wv_hamming_hist": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _vp, _sz, _vp]),
    "wv_hamming_topk_rows16": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _sz, _vp]),
    "wv_hamming_shard_relbits": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _i, _i64, _i, _i, _vp]),
    "wv_merge_relbits_map": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "wv_hamming_shard_prefix": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _sz, _vp]),
    "wv_topk_merge": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "wv_rank_from_dist": (_i, [_vp, _i64, _i, _i64, _i, _vp, _vp, _i, _vp]),
    "wv_map_at_k": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "wv_map_at_k_ld": (_i, [_vp, _i64, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "wv_hamming_map_at_ks": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _i, _vp, _vp, _vp]),
    "wv_merge_relbits_map_ks": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "wv_merge_relbits_map_ks_lds_bytes": (_sz, [_i, _i, _i]),
    "wv_map_at_ks": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "wv_map_at_ks_cpu": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "wv_label_overlap_hist": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp]),
    "wv_label_overlap_hist_cpu": (_i, [_vp, _vp, _i, _i, _i64, _vp]),
    "wv_ndcg_weights": (_i, [_vp, _i64]),
    "wv_ndcg_at_ks": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "wv_ndcg_at_ks_cpu": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "wv_topk_merge_cum": (_i, [_vp, _vp, _i, _i, _i, _i64, _vp, _vp, _i, _i, _vp]),
    "wv_topk_merge_cum_need": (_i, [_vp, _vp, _i, _i, _i, _i64, _vp, _vp, _i, _i, _vp, _vp]),
    "wv_hit_prefix": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "wv_knn_float_workspace_bytes": (_sz, [_i, _i64, _i, _i]),
    "wv_knn_float": (_i, [_vp, _vp, _i, _i64, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "wv_band_attn_pool_workspace_bytes": (_sz, [ctypes.POINTER(HeadParams), _i]),
    "wv_band_attn_qproj": (_i, [ctypes.POINTER(HeadParams), _vp, _vp]),
    "wv_band_attn_prepared_bytes": (_sz, [ctypes.POINTER(HeadParams)]),
    "wv_band_attn_prepare": (_i, [ctypes.POINTER(HeadParams), _vp, _vp]),
    "wv_band_attn_pool": (_i, [ctypes.POINTER(HeadParams), _vp, _i, _vp, _vp, _sz, _vp]),
    "wv_hash_tail": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp]),
    "wv_knn_float_cpu": (_i, [_vp, _vp, _i, _i64, _i, _i, _i, _vp, _vp]),
    "wv_rank_scores_workspace_bytes": (_sz, [_i, _i64, _i]),
    "wv_rank_scores": (_i, [_vp, _i, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "wv_rank_scores_cpu": (_i, [_vp, _i, _i64, _i, _i, _vp, _vp]),
    "wv_band_attn_pool_cpu": (_i, [ctypes.POINTER(HeadParams), _vp, _i, _vp]),
    "wv_hash_tail_cpu": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp]),
    "wv_band_attn_bf16_prepared_bytes": (_sz, [ctypes.POINTER(HeadParams)]),
    "wv_band_attn_bf16_prepare": (_i, [ctypes.POINTER(HeadParams), _vp, _vp]),
    "wv_band_attn_pool_bf16_workspace_bytes": (_sz, [ctypes.POINTER(HeadParams), _i]),
    "wv_band_attn_pool_bf16": (_i, [ctypes.POINTER(HeadParams), _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "wv_band_attn_pool_bf16_cpu": (_i, [ctypes.POINTER(HeadParams), _vp, _i, _i, _vp]),
    "wv_band_attn_maps_workspace_bytes": (_sz, [ctypes.POINTER(HeadParams), _i]),
    "wv_band_attn_maps": (_i, [ctypes.POINTER(HeadParams), _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wv_band_attn_maps_cpu": (_i, [ctypes.POINTER(HeadParams), _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "wv_image_size": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "wv_image_size_cpu": (_i, [_vp, _vp, _vp, _i]),
    "wv_image_size_check": (_i, [_vp, _i]),
    "wv_colour_jitter_workspace_bytes": (_sz, [_i]),
    "wv_colour_jitter": (_i, [_vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "wv_colour_jitter_cpu": (_i, [_vp, _vp, _i]),
    "wv_colour_jitter_check": (_i, [_vp, _i]),
    "wv_lift_out_size": (_i, [_i, _i, _i]),
    "wv_lift_images_tile": (_i, [_i]),
    "wv_lift_images_check": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "wv_lift_images_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "wv_lift_images": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "wv_lift_images_cpu": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _fp, _fp, _i, _i, _i, _vp]),
    "wv_group_layernorm_check": (_i, [_i, _i, _i64, _i64, _i, _i]),
    "wv_group_layernorm": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i, _i, _vp, _vp, _f, _vp]),
    "wv_group_layernorm_cpu": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i, _i, _vp, _vp, _f]),
    "wv_ip_map_at_k": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "wv_ip_map_at_k_cpu": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "wv_pair_loss_workspace_bytes": (_sz, [_i, _i]),
    "wv_pair_loss": (_i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(PairLossParams), _vp, _vp, _vp, _sz, _vp]),
    "wv_pair_loss_cpu": (_i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(PairLossParams), _vp, _vp]),
    "wv_rank_ap_workspace_bytes": (_sz, [_i, _i, _i]),
    "wv_rank_ap": (_i, [_vp, _vp, _i, _i, ctypes.POINTER(RankApParams), _vp, _vp, _vp, _sz, _vp]),
    "wv_rank_ap_cpu": (_i, [_vp, _vp, _i, _i, ctypes.POINTER(RankApParams), _vp, _vp]),
}

_LIB = None
_DIAG = None
_USE_DIAG = os.environ.get("WVHASH_DIAG") == "1"      # tools/: run a whole script on the diagnostic build


def _open(path):
    if not os.path.exists(path):
        raise WvhashUnavailable(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C image-retrieval-wavelet_amd/csrc`. There is no CPU fallback.")
    # torch ships its own libamdhip64 (same SONAME as /opt/rocm's): make sure it is the one mapped
    hip_in_torch = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip_in_torch):
        ctypes.CDLL(hip_in_torch, mode=ctypes.RTLD_GLOBAL)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise WvhashUnavailable(f"cannot load {path}: {e}") from e
    lib.wv_abi_version.restype = ctypes.c_int
    have = lib.wv_abi_version()
    if have != ABI_VERSION:
        raise WvhashUnavailable(f"{path} reports ABI {have}, this package binds ABI {ABI_VERSION}: rebuild it "
                                "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libwvhash.so (after torch, so that both share one HIP runtime)."""
    global _LIB, _DIAG
    if _USE_DIAG:
        if _DIAG is None:
            _DIAG = _open(DIAG_LIB_PATH)
        return _DIAG
    if _LIB is None:
        _LIB = _open(LIB_PATH)
    return _LIB


@contextlib.contextmanager
def diagnostic():
    """Inside the block every op goes through libwvhash_diag.so, whose entry points honour the WV_* kernel-selection
    switches (tests pin each code path with them; tools/ A/B variants).  Never used by the product path."""
    global _USE_DIAG
    prev, _USE_DIAG = _USE_DIAG, True
    try:
        yield load()
    finally:
        _USE_DIAG = prev


def require_gpu():
    if not torch.cuda.is_available():
        raise WvhashUnavailable("wvhash ops need a ROCm GPU (torch.cuda.is_available() is False); "
                                "there is no CPU fallback in the product path")
    return load()


def check(rc, what="", unsupported=False):
    """unsupported: the caller has another way to the same result, so WV_ENOTSUP is a WvhashUnsupported of its own"""
    if rc != 0:
        msg = load().wv_last_error().decode(errors="replace")
        if unsupported and rc == WV_ENOTSUP:
            raise WvhashUnsupported(f"{what}: {msg}")
        if rc == -22:
            raise ValueError(f"{what}: {msg}")
        raise WvhashError(f"{what}: rc={rc}: {msg}")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def wv_band_attn_maps(p, feats, layout, B, probs=None, probs_mean=None, scores=None, attn_out=None):
    """The attention maps of the head into the given fp32 tensors (None = not wanted): wv_band_attn_maps on the stream of
    `feats`' GPU with a workspace of its own, or the host twin wv_band_attn_maps_cpu when `feats` is a host tensor.  Every
    pointer of `p` must live where `feats` does."""
    outs = [ptr(t) for t in (probs, probs_mean, scores, attn_out)]
    if not feats.is_cuda:
        return check(load().wv_band_attn_maps_cpu(ctypes.byref(p), ptr(feats), layout, B, *outs), "wv_band_attn_maps_cpu")
    lib = require_gpu()
    with torch.cuda.device(feats.device):
        nbytes = lib.wv_band_attn_maps_workspace_bytes(ctypes.byref(p), B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=feats.device)
        rc = lib.wv_band_attn_maps(ctypes.byref(p), ptr(feats), layout, B, *outs, ptr(ws), ctypes.c_size_t(nbytes), stream_ptr())
    check(rc, "wv_band_attn_maps", unsupported=True)


def host_floats(values):
    arr = (ctypes.c_float * len(values))(*[float(v) for v in values])
    return arr
