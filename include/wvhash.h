/*
 * wvhash.h -- C ABI of libwvhash.so, the MI355X (gfx950) implementation of the
 * wavelet-hashing retrieval hot path of ArseneAmoya/image-retrieval-wavelet.
 *
 * The reference is pure Python; its FFI boundary for this path is "Python calls into a native
 * wheel" (PyWavelets for the transform, ATen / faiss for the ranking, ATen for the attention
 * head).  Each entry point below names the reference call site it replaces (file:line under
 * /root/reference) -- the ctypes binding a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns 0 (WV_OK) or a negative errno-style code; nothing throws across
 *     the ABI.  wv_last_error() returns a per-thread message for the last failure.
 *   - All pointers are DEVICE pointers unless the name says host.  The caller owns every
 *     buffer; the library allocates nothing.  Scratch comes from the caller, sized by the
 *     matching *_workspace_bytes() query.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue
 *     work: no hidden synchronisation, no host<->device copies.
 *   - Thread-safe and re-entrant; no global mutable state except the per-thread error string.
 *   - One process per GPU; the current HIP device of the calling thread is used.
 *   - Alignment.  For the ranking, metric and loss entry points (wv_hamming_dist ... wv_hit_prefix, wv_ip_map_at_k,
 *     wv_group_layernorm, wv_pair_loss, wv_rank_ap) every typed pointer needs the natural alignment of its element and no
 *     more: 1 byte for uint8 distance rows and matrices, 2 for uint16 rows and bf16, 4 for int32 / uint32 / float, 8 for
 *     uint64 / double.  Kernels that move 16 bytes at a time test the address (and the row pitch) at run time and take an
 *     element-wise path otherwise: the same bits at any alignment.  The exception is opaque memory: every `workspace`,
 *     `prepared` and `prepared_labels` of these entry points holds images the kernels read and write as 16-byte words and
 *     must be 16-BYTE ALIGNED; anything else is WV_EINVAL, answered on the host before any launch, no buffer touched.
 *     (wv_knn_float states its own 16 bytes below.)  tests/test_gpu_buffer_contract.py holds the entry points to this.
 */
#ifndef WVHASH_H
#define WVHASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WV_OK 0
#define WV_EINVAL (-22)  /* bad argument (message says which) */
#define WV_ENOMEM (-12)  /* workspace too small */
#define WV_ENOTSUP (-95) /* shape outside what the kernels implement */
#define WV_EHIP (-5)     /* HIP runtime error at launch */

/* element types of image / coefficient buffers */
#define WV_DT_U8 0
#define WV_DT_F32 1
#define WV_DT_BF16 2

/* image memory layouts */
#define WV_LAYOUT_NCHW 0 /* [B][C][H][W]  (torch, after ToTensor-style permute) */
#define WV_LAYOUT_NHWC 1 /* [B][H][W][C]  (PIL / numpy, what np.array(img) yields) */

const char *wv_last_error(void);
/* 5 = this header.  History: the bf16 head entry points (wv_band_attn_bf16_prepare ... wv_band_attn_pool_bf16_cpu) were added
 * under 5 -- new symbols only, no struct or existing signature changed; 5 added WV_METRIC_L2_SQUARED, wv_rank_scores[_cpu] and the host twins wv_knn_float_cpu,
 * wv_band_attn_pool_cpu, wv_hash_tail_cpu; 4 added the host twins of the ranking side (wv_pack_bits_cpu ... wv_hit_prefix_cpu); 2 added wv_head_params.q_proj, the host twins, wv_swt2d_forward_ex, the two-step shard entry
 * points and wv_map_at_k_ld; 3 added wv_head_params.prepared / wv_band_attn_prepare (one-launch head front), the ranking + AP
 * entry points (wv_hamming_map_at_k, wv_rank_labels_prepare), wv_hamming_shard_prefix / wv_topk_merge_cum_need and the
 * relevance-string pair of the sharded mAP (wv_hamming_shard_relbits, wv_merge_relbits_map).  The multi-cut-off entry points
 * (wv_hamming_map_at_ks, wv_merge_relbits_map_ks[_lds_bytes], wv_map_at_ks, wv_map_at_ks_cpu) were added under 5 as well: new symbols only.
 * So were the radius histograms (wv_hamming_radius_hist, wv_hamming_radius_hist_cpu): 71 symbols.
 * So were the NDCG entry points (wv_label_overlap_hist[_cpu], wv_ndcg_weights, wv_ndcg_at_ks[_cpu]): 76 symbols.
 * So were the attention maps of the head (wv_band_attn_maps[_workspace_bytes], wv_band_attn_maps_cpu): 79 symbols.
 * So was the image sizing (wv_image_size, wv_image_size_cpu, wv_image_size_check, struct wv_size_stage): 82 symbols.
 * So was the colour jitter (wv_colour_jitter[_workspace_bytes], wv_colour_jitter_cpu, wv_colour_jitter_check, struct
 * wv_colour_ops): 86 symbols.
 * So was the batched lifting tail (wv_lift_images[_workspace_bytes], wv_lift_images_cpu, wv_lift_images_check,
 * wv_lift_out_size, wv_lift_images_tile): 92 symbols.
 * So was the single-band SWT (wv_swt2d_band_forward, wv_swt2d_band_forward_cpu): 94 symbols.
 * So was the grouped LayerNorm (wv_group_layernorm, wv_group_layernorm_cpu, wv_group_layernorm_check): 97 symbols.
 * So was the batch mAP proxy of real-valued embeddings (wv_ip_map_at_k, wv_ip_map_at_k_cpu): 99 symbols.
 * So were the pairwise hashing losses (wv_pair_loss[_workspace_bytes], wv_pair_loss_cpu, struct wv_pair_loss_params): 102 symbols.
 * So were the rank-approximation AP losses (wv_rank_ap[_workspace_bytes], wv_rank_ap_cpu, struct wv_rank_ap_params): 105 symbols.
 * A struct gaining a field bumps it. */
int wv_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Stationary wavelet transform.
 * Replaces pywt.swt2(channel, wavelet, level)[0] + np.stack + the /255 scaling of
 *   main/transforms/custom_transforms.py:145-157 (BaseWaveletTransform.__call__) and
 *   :163-166 (SWTTransform._apply_wavelet), for a whole batch at once.
 * in : [B,C,H,W] or [B,H,W,C]; u8 values are divided by 255.0f, f32 values are used as is.
 * out: [B][C][4][H][W], band order cA, cH, cV, cD of level `level` (coarsest) only.
 * H and W must be multiples of 2^level (PyWavelets raises otherwise -> WV_EINVAL).
 * dec_lo / dec_hi: HOST pointers to `flen` decomposition taps (PyWavelets order).
 * workspace: needed only for shapes the tiled kernel does not cover (query below; may be 0).
 * ------------------------------------------------------------------------------------------ */
size_t wv_swt2d_workspace_bytes(int B, int C, int H, int W, int level, int flen);
int wv_swt2d_forward(const void *in, int in_dtype, int in_layout, void *out, int out_dtype, int B,
                     int C, int H, int W, int level, const float *dec_lo, const float *dec_hi,
                     int flen, void *workspace, size_t workspace_bytes, void *stream);

/* Same transform with a choice of output layout.
 *   WV_BANDS_INNER: out [B][C][4][H][W] -- the reference's tensor (custom_transforms.py:155-157, batched).
 *   WV_BANDS_OUTER: out [4][B'][C][H][W], band_stride = B'*C*H*W elements between the bands of one plane
 *                   (B' >= B: a chunk of a larger batch may be written in place).  Every band is then one
 *                   contiguous NCHW batch: exactly what SharedDinoHashing.forward builds with
 *                   x.permute(2,0,1,3,4).contiguous().view(4B,3,H,W) (multi_dino_attention.py:818) and what
 *                   MultiDinoHashing indexes per backbone (:745) -- written directly, without that second copy of
 *                   the sub-band tensor.  Returns WV_ENOTSUP for shapes only the tiled/generic kernels cover. */
#define WV_BANDS_INNER 0
#define WV_BANDS_OUTER 1
int wv_swt2d_forward_ex(const void *in, int in_dtype, int in_layout, void *out, int out_dtype, int out_layout,
                        int64_t band_stride, int B, int C, int H, int W, int level, const float *dec_lo,
                        const float *dec_hi, int flen, void *workspace, size_t workspace_bytes, void *stream);

/* One band of the same transform as a plain image batch: what a single-band model reads
 *   (main/models/detail_tester.py:36,100: x[:, :, detail_index, :, :]) without the other three bands being
 *   computed or written.
 * band: 0..3 = cA, cH, cV, cD -- the order wv_swt2d_forward writes, the reference's detail_index.
 * out : [B][C][H][W], f32 or bf16.  Every element equals the same element of wv_swt2d_forward's band bit for bit.
 * Implemented for the shapes of the sliding kernel (the hot path) only: any other shape returns WV_ENOTSUP, the
 * message quoting the rule the shape breaks, and the caller slices wv_swt2d_forward's result.  No workspace.
 * Arguments are checked on the host before anything touches the GPU: band outside 0..3 -> WV_EINVAL. */
int wv_swt2d_band_forward(const void *in, int in_dtype, int in_layout, void *out, int out_dtype, int band,
                          int B, int C, int H, int W, int level, const float *dec_lo, const float *dec_hi,
                          int flen, void *stream);

/* RawStackTransform (custom_transforms.py:172-188): `copies` identical planes per channel.
 * out: [B][C][copies][H][W].  in_layout other than WV_LAYOUT_NCHW / WV_LAYOUT_NHWC -> WV_EINVAL, before any launch. */
int wv_rawstack_forward(const void *in, int in_dtype, int in_layout, void *out, int out_dtype,
                        int B, int C, int H, int W, int copies, void *stream);

/* ------------------------------------------------------------------------------------------
 * Host twins of the three transform entry points ("_cpu twins taking host pointers").
 * The reference calls its transform inside forked DataLoader worker processes, one image at a time
 *   (main/datasets/flikr_coco.py:59-60 -> custom_transforms.py:145-157); a forked worker cannot use the parent's
 *   GPU context, so with an unchanged transform YAML and num_workers > 0 the plugin's __call__ runs these.
 * in / out are HOST pointers; out is float32 [B][C][4|copies][H'][W'] like the device entry points.
 * No HIP call, no thread started, no global state: safe after fork().  Float32 arithmetic in the order of the
 * device kernels (bit-identical to wv_swt2d_forward on the shapes its sliding kernel covers).
 * ------------------------------------------------------------------------------------------ */
int wv_swt2d_forward_cpu(const void *in, int in_dtype, int in_layout, float *out, int B, int C, int H, int W,
                         int level, const float *dec_lo, const float *dec_hi, int flen);
/* Host twin of wv_swt2d_band_forward: out is float32 [B][C][H][W]; every shape wv_swt2d_forward_cpu covers, each
 * element equal to the same element of its band bit for bit. */
int wv_swt2d_band_forward_cpu(const void *in, int in_dtype, int in_layout, float *out, int band,
                              int B, int C, int H, int W, int level, const float *dec_lo, const float *dec_hi, int flen);
int wv_rawstack_forward_cpu(const void *in, int in_dtype, int in_layout, float *out, int B, int C, int H, int W,
                            int copies);
int wv_dwt2d_forward_cpu(const void *in, int in_dtype, int in_layout, float *out, int B, int C, int H, int W,
                         int level, const float *dec_lo, const float *dec_hi, int flen);

/* ------------------------------------------------------------------------------------------
 * Host twins of the ranking-side entry points (BASELINE config c0 is the CPU plumbing case).
 * The reference's calculator runs on CPU tensors (main/engine/accuracy_calculator.py:279-349 with self.device = cpu,
 *   main/engine/evaluate.py:76-81); CustomCalculator(device='cpu') -- explicit, never a silent fallback -- runs these.
 * All pointers are HOST pointers; argument meaning as for the device entry point of the same name (no stream, no
 * workspace).  Same results bit for bit: packed words, counts, distances and the (distance, row) order are integers; the
 * average precision sums its fp32 quotients in wv_map_at_k's order.  No HIP call, no thread, no global state.
 *   wv_pack_bits_cpu     <- wv_pack_bits        wv_bit_counts_cpu   <- wv_bit_counts     wv_hamming_dist_cpu <- wv_hamming_dist
 *   wv_hamming_topk_cpu  <- wv_hamming_topk (stable counting sort; dist may be NULL)
 *   wv_map_at_k_cpu      <- wv_map_at_k_ld      wv_hit_prefix_cpu   <- wv_hit_prefix
 * ------------------------------------------------------------------------------------------ */
int wv_pack_bits_cpu(const float *src, int64_t ld_src, uint64_t *packed, int64_t rows, int nbits, int mode, int32_t *bad_flag);
int wv_bit_counts_cpu(const uint64_t *packed, int64_t rows, int nbits, uint32_t *counts);
int wv_hamming_dist_cpu(const uint64_t *q, const uint64_t *db, uint8_t *dist, int64_t ld_dist, int Q, int64_t N, int words);
int wv_hamming_topk_cpu(const uint64_t *q, const uint64_t *db, int32_t *idx, uint8_t *dist, int Q, int64_t N, int nbits, int k,
                        int64_t idx_offset);
int wv_map_at_k_cpu(const int32_t *idx, int64_t ld, int Q, int k, const uint64_t *qlab, const uint64_t *dblab, int lwords,
                    float *ap, int32_t *nrel);
int wv_hit_prefix_cpu(const int32_t *idx, int Q, int k, const uint64_t *qlab, const uint64_t *dblab, int lwords, uint32_t *hits);

/* Decimated multi-level 2-D DWT (DWTTransform, custom_transforms.py:191-205 -> pywt.wavedec2, mode
 * 'symmetric'): the four bands (cA, cH, cV, cD) of the coarsest level.
 * out: float32 [B][C][4][Hn][Wn] with Hn = wv_dwt_out_len(H, flen, level) (each level: floor((n + flen - 1) / 2)).
 * Arguments are checked on the host before any launch: level outside 1..12, flen outside 2..32, an unknown dtype or
 * layout -> WV_EINVAL; a workspace smaller than wv_dwt2d_workspace_bytes reports -> WV_ENOMEM. */
int wv_dwt_out_len(int n, int flen, int level);
size_t wv_dwt2d_workspace_bytes(int B, int C, int H, int W, int level, int flen);
int wv_dwt2d_forward(const void *in, int in_dtype, int in_layout, float *out, int B, int C, int H, int W,
                     int level, const float *dec_lo, const float *dec_hi, int flen, void *workspace,
                     size_t workspace_bytes, void *stream);

/* One level of the legacy lifting-scheme DWT behind CustomTransform (custom_transforms.py:14-55,90-117;
 * wavelets/haar.py:21-86, wavelets/cdf_97.py:33-133): basis 0 = haar, 1 = cdf 9/7, zero-padded lifting steps,
 * 2-D scales (1/2, 1, 1, sqrt 2).  in: float32 [planes][H][W], H and W even (the caller pads like
 * HaarLifting / Cdf97Lifting do);  ll: [planes][H/2][W/2];  hi: [planes][3][H/2][W/2] = (LH, HL, HH).
 * Bit-identical to the reference's float32 torch ops (every product and sum rounded separately, same order).
 * One plane-sized fp32 workspace, two launches, all four bands of ONE level of already padded planes: the per-image
 * building block behind HaarLifting / Cdf97Lifting.  A whole pipeline tail (ToTensor -> Normalize -> CustomTransform) on a
 * batch is wv_lift_images below; both compile the same lifting chain (csrc/lifting.hpp). */
size_t wv_lifting2d_workspace_bytes(int64_t planes, int H, int W);
int wv_lifting2d_forward(const float *in, int64_t planes, int H, int W, int basis, float *ll, float *hi,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The tensor tail of the legacy configs for a whole batch: ToTensor -> [Normalize] -> [CustomTransform(levels, basis,
 * coarse_only=True, ll_only)] on the sized images, bit-identical to the reference's float32 torch ops.
 * in     [B][C][H][W] (WV_LAYOUT_NCHW) or [B][H][W][C] (WV_LAYOUT_NHWC, what wv_image_size writes), tightly packed.
 *        WV_DT_U8: each byte x of channel c becomes  t = (float)x / 255.0f  when to_tensor = 1 ((float)x when 0), then
 *        v = (t - mean[c]) / std[c]  when mean / std are given: a true division, a subtraction and a true division, each
 *        rounded to fp32 -- ToTensor's .div(255), Normalize's sub_ / div_.  mean, std: HOST pointers to C floats each,
 *        both NULL = no Normalize.  WV_DT_F32: the values are used as they are (to_tensor = 0, mean = std = NULL).
 * levels >= 1: per level the plane is taken as zero-padded at the right and bottom (haar: to even sizes, cdf 9/7: to
 *        multiples of 4; the pad is +0.0 and comes AFTER Normalize; nothing is padded in memory), then one 2-D lifting level
 *        as wv_lifting2d_forward defines it.  Only the approximation feeds the next level.
 * out    float32, h = wv_lift_out_size(H, basis, levels), w likewise:
 *        levels >= 1, ll_only = 0: [B][C][4][h][w] = (LL, LH, HL, HH) of the coarsest level
 *        levels >= 1, ll_only = 1: [B][C][h][w]
 *        levels  = 0             : [B][C][H][W], the conversion alone (ll_only is not looked at)
 * wv_lift_images            one launch per level on `stream`; a non-final level stores its LL planes alone into the
 *                           workspace (wv_lift_images_workspace_bytes: 0 for levels <= 1; a shorter one is WV_ENOMEM,
 *                           answered before any launch).  No hidden synchronisation, no allocation, no copy.
 * wv_lift_images_cpu        host twin (HOST pointers, single-threaded, no HIP call): the same bits.
 * wv_lift_images_check      the one argument check of both.  WV_EINVAL: an unknown dtype / layout / basis, B < 0, C, H or
 *                           W < 1, levels < 0, ll_only outside {0, 1}.  WV_ENOTSUP, the kernel's limits: C > 4, H or W >
 *                           16384, levels > 16, B * C > 2^31 - 1.  Both entry points add: to_tensor outside {0, 1}, mean
 *                           without std, to_tensor = 1 on float32 input, a std of 0 or a NaN (WV_EINVAL); Normalize on
 *                           float32 input (WV_ENOTSUP: it is folded into the 256-entry byte table only).
 * wv_lift_out_size          length of one axis after `levels` levels (0 for arguments the check refuses).
 * wv_lift_images_tile       input samples per workgroup tile along H (axis 0) and W (axis 1), for tests that place sizes
 *                           around the tile edges. */
int wv_lift_out_size(int n, int basis, int levels);
int wv_lift_images_tile(int axis);
int wv_lift_images_check(int in_dtype, int in_layout, int B, int C, int H, int W, int basis, int levels, int ll_only);
size_t wv_lift_images_workspace_bytes(int B, int C, int H, int W, int basis, int levels);
int wv_lift_images(const void *in, int in_dtype, int in_layout, int B, int C, int H, int W, int to_tensor,
                   const float *mean, const float *std, int basis, int levels, int ll_only, float *out, void *workspace,
                   size_t workspace_bytes, void *stream);
int wv_lift_images_cpu(const void *in, int in_dtype, int in_layout, int B, int C, int H, int W, int to_tensor,
                       const float *mean, const float *std, int basis, int levels, int ll_only, float *out);

/* ------------------------------------------------------------------------------------------
 * Bit packing of +-1 hash codes and multi-hot labels.
 * Codes come out of torch.sign(logits) (multi_dino_attention.py:833) as fp32 in {-1,+1};
 * the reference keeps them as fp32 rows and multiplies (accuracy_calculator.py:183-186).
 * packed[row][w] bit j  =  src[row][64*w + j] > 0.      words = ceil(nbits / 64).
 * mode 0 (codes): *bad_flag |= 1 if any value is not exactly +1 or -1 (sign(0)=0, NaN ...)
 * mode 1 (labels): *bad_flag |= 1 if any value is negative or NaN (then "q.r > 0" is no longer
 *                  "shares a tag" and label_comparison_fn :31-37 cannot be evaluated on bits).
 * bad_flag: device int32, caller zero-initialises; may be NULL.
 * ------------------------------------------------------------------------------------------ */
int wv_pack_bits(const float *src, int64_t ld_src, uint64_t *packed, int64_t rows, int nbits,
                 int mode, int32_t *bad_flag, void *stream);

/* Per-bit population counts over the rows (per_bit_balance, accuracy_calculator.py:188-194:
 * (reference > 0).float().mean(0) = counts / rows).  counts: device uint32[nbits], zeroed here. */
int wv_bit_counts(const uint64_t *packed, int64_t rows, int nbits, uint32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hamming distances.  Replaces calc_hamming_dist (accuracy_calculator.py:183-186),
 * 0.5 * (B - q @ r.T), for +-1 codes, where it is an exact small integer.
 * dist[qi * ld_dist + n] = popcount(q[qi] ^ db[n]),  uint8 (nbits <= 255).
 * q, db: 8-byte aligned (a row slice of a larger database is fine); dist: any address, any ld_dist >= N.
 * ------------------------------------------------------------------------------------------ */
int wv_hamming_dist(const uint64_t *q, const uint64_t *db, uint8_t *dist, int64_t ld_dist, int Q,
                    int64_t N, int words, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused Hamming distance + ranking: the k nearest database codes of every query in ascending
 * (distance, database index) order -- the canonical tie-break of torch.argsort(stable=True).
 * Replaces  hamm = calc_hamming_dist(...); indices = torch.argsort(hamm)[:topk]
 *   (accuracy_calculator.py:219-223) and get_knn_torch's  q @ r.T + torch.topk(largest=True)
 *   (get_knn.py:63-66; IP score = nbits - 2 * dist), and faiss IndexFlatIP.search (:35-52).
 * idx : int32 [Q][k], values = local row + idx_offset (idx_offset = first global row of this
 *       shard when the database is row-sharded across GPUs).
 * dist: uint8 [Q][k], or NULL when only the lists are wanted (the lists have the same bits).   Requires 1 <= k <= N, nbits <= 128.
 * idx 4-byte aligned, dist at any address (any k: the rows of odd k start at every residue);  workspace: 16-byte aligned,
 * wv_hamming_topk_workspace_bytes() bytes, written before it is read (old content is never looked at).
 * ------------------------------------------------------------------------------------------ */
size_t wv_hamming_topk_workspace_bytes(int Q, int64_t N, int words, int k);
int wv_hamming_topk(const uint64_t *q, const uint64_t *db, int32_t *idx, uint8_t *dist, int Q,
                    int64_t N, int nbits, int k, int64_t idx_offset, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Prepared database.  The reference rebuilds a faiss index on every call (index.add, get_knn.py:54);
 * here the per-database work is explicit: wv_db_prepare lays the packed codes out once in the two
 * images the kernels read with fully coalesced loads (distance tile image + ranking column image),
 * and the *_prepared entry points skip the per-call re-layout.  Results are identical to the
 * plain entry points.  `prepared` is caller-owned device memory of wv_db_prepared_bytes() bytes, 16-byte aligned (WV_EINVAL
 * otherwise, here and in every entry point that reads it); wv_db_prepare writes every byte a reader looks at.  db: 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
size_t wv_db_prepared_bytes(int64_t N, int words);
int wv_db_prepare(const uint64_t *db, int64_t N, int words, void *prepared, size_t prepared_bytes,
                  void *stream);
int wv_hamming_dist_prepared(const uint64_t *q, const void *prepared, uint8_t *dist, int64_t ld_dist,
                             int Q, int64_t N, int words, void *stream);
int wv_hamming_topk_prepared(const uint64_t *q, const void *prepared, int32_t *idx, uint8_t *dist, int Q,
                             int64_t N, int nbits, int k, int64_t idx_offset, void *stream);

/* Same ranking with every option: `prepared` (or NULL) instead of / beside `db`, and `cum` (or NULL):
 * uint32 [Q][nbits + 2] (4-byte aligned), cum[q][b] = number of database rows of THIS call with distance < b (cum[q][nbits+1] = N).
 * A row-sharded search all-reduces `cum` to learn each query's global k-th distance, and then exchanges only
 * the list prefixes that can matter (wvhash/parallel.py) -- the role faiss' host-side shard merge plays at
 * get_knn.py:41-44. */
int wv_hamming_topk_ex(const uint64_t *q, const uint64_t *db, const void *prepared, int32_t *idx, uint8_t *dist,
                       uint32_t *cum, int Q, int64_t N, int nbits, int k, int64_t idx_offset, void *workspace,
                       size_t workspace_bytes, void *stream);

/* mAP@k of every query straight from the codes -- what calculate_maphashing (accuracy_calculator.py:183-231) returns -- without
 * writing the ranked lists: the windowed ranking kernel builds the list in LDS as wv_hamming_topk does (ascending distance,
 * ties by ascending row) and evaluates it there against a relevance bitmap of the query made from the rows' label words
 * (lwords = 1 or 2 64-bit multi-hot words per row, i.e. up to 128 classes: label_comparison_fn, :31-37).  ap float32 [Q] and nrel int32 [Q] (or NULL) are exactly
 * what wv_map_at_k returns for wv_hamming_topk's list (same summation order; bit-identical at 256 threads per query).
 *   prepared         wv_db_prepare's blob of the database codes
 *   prepared_labels  wv_rank_labels_prepare's class-major bit matrix of the rows' label words
 *                    (wv_rank_labels_prepared_bytes(N) bytes; 0 = N is outside the windowed kernel); 16-byte aligned like `prepared`
 * Returns WV_ENOTSUP for shapes outside the fused kernel (more than 32,768 rows, k > 32,639 -- the list is built in LDS with
 * 16-bit cells --, lists that do not fit LDS beside the label bitmap, ...; mAP@ALL with k = N is inside for N <= 32,639): the caller then runs
 * wv_hamming_topk + wv_map_at_k. */
size_t wv_rank_labels_prepared_bytes(int64_t N, int lwords);
int wv_rank_labels_prepare(const uint64_t *dblab, int64_t N, int lwords, void *prepared_labels, size_t prepared_bytes, void *stream);
int wv_hamming_map_at_k(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab, int lwords,
                        int Q, int64_t N, int nbits, int k, float *ap, int32_t *nrel, void *stream);

/* The two steps of a row-sharded search (wvhash/parallel.py; the role of faiss' shard search + host merge at
 * get_knn.py:41-44) on one shard of at most 32,768 rows:
 *   wv_hamming_hist        only the cumulative distance histogram of every query, cum uint32 [Q][nbits + 2] as above -- no
 *                          list is built.  All-reduced over the shards it gives every rank the global k-th distance of every
 *                          query, hence how long a list prefix each shard has to contribute (about k / shards + ties).
 *   wv_hamming_topk_rows16 the k nearest rows of the shard per query in (distance, row) order as 16-bit LOCAL row numbers,
 *                          uint16 [Q][k] -- the wire format wv_topk_merge_cum reads -- with k = that prefix length.
 * Returns WV_ENOTSUP for shards outside the windowed kernel's range (the caller then uses wv_hamming_topk_ex).
 * rows: 2-byte aligned (odd k: the rows of odd queries start at 2 mod 4), cum: 4-byte aligned; workspace / prepared: 16 bytes. */
int wv_hamming_hist(const uint64_t *q, const uint64_t *db, const void *prepared, uint32_t *cum, int Q, int64_t N, int nbits,
                    void *workspace, size_t workspace_bytes, void *stream);
int wv_hamming_topk_rows16(const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows, int Q, int64_t N,
                           int nbits, int k, void *workspace, size_t workspace_bytes, void *stream);
/* Both in one pass, for a steady stream of query batches whose prefix length is known from earlier batches (wvhash/parallel.py
 * with send_hint): the shard's k nearest rows per query as 16-bit local row numbers AND its complete cumulative histograms.
 * No all-reduce is needed before the lists can be built; whether k was enough is checked by the receiver of the lists
 * (wv_topk_merge_cum_need). */
int wv_hamming_shard_prefix(const uint64_t *q, const uint64_t *db, const void *prepared, uint16_t *rows, uint32_t *cum, int Q,
                            int64_t N, int nbits, int k, void *workspace, size_t workspace_bytes, void *stream);

/* Merge of G per-shard top-k lists (gathered with one all-gather) into the global top-k.
 * Replaces the host-side shard merge inside faiss.index_cpu_to_all_gpus(shards=True)
 *   (get_knn.py:41-44).  Lists must come from contiguous row shards in rank order, so that
 * ascending global index inside a distance bucket = (shard, position) order.
 * idx_in/dist_in: [G][Q][kin];  idx_out/dist_out: [Q][k], k <= G*kin. nbits <= 128.
 * Shorter lists are padded with dist = nbits + 1 (idx = -1): such entries rank after every real one. */
int wv_topk_merge(const int32_t *idx_in, const uint8_t *dist_in, int G, int Q, int kin,
                  int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream);

/* Compact merge for the sharded search: every shard sends, per query, its cumulative distance histogram
 * (cum, uint32 [G][Q][nbits + 2], the `cum` output of wv_hamming_topk_ex: rows with distance < b) instead of a
 * distance row, and its list as 16-bit LOCAL row numbers (idx_local uint16 [G][Q][kin], shard_rows <= 65536;
 * shard g holds global rows [g * shard_rows, ...)).  A sorted list is fully described by its histogram.
 * Output as wv_topk_merge.  Replaces the host merge of faiss' sharded index (get_knn.py:41-44) with 2.2x fewer
 * exchanged bytes than int32 indices + uint8 distances. */
int wv_topk_merge_cum(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin, int64_t shard_rows,
                      int32_t *idx_out, uint8_t *dist_out, int k, int nbits, void *stream);
/* The same merge; additionally need_out[0] = max(need_out[0], the longest prefix any shard had to contribute for a query of
 * this launch) -- from the unclamped histograms: the merged lists are exact iff that value is <= kin.  The caller zeroes
 * need_out beforehand and looks at it whenever it synchronises anyway. */
int wv_topk_merge_cum_need(const uint16_t *idx_local, const uint32_t *cum, int G, int Q, int kin, int64_t shard_rows,
                           int32_t *idx_out, uint8_t *dist_out, int k, int nbits, int32_t *need_out, void *stream);

/* Sharded mAP@k without lists on the wire (wvhash/parallel.py: sharded_hamming_map_at_k).  calculate_maphashing needs, of every
 * list entry, only whether it is relevant: a shard therefore sends per query the RELEVANCE STRING of its k nearest rows (bit p
 * = its p-th nearest row shares a label with the query; 1 bit per entry instead of a 16-bit row number) and its cumulative
 * histogram; the receiver interleaves the strings of the G shards bin by bin (global order = distance, shard, position) and
 * evaluates the merged string exactly as wv_map_at_k evaluates a list.
 *   wv_hamming_shard_relbits  relbits uint64 [Q][ceil(k / 64)], cum uint32 [Q][nbits + 2]; prepared / prepared_labels: the
 *                             shard's wv_db_prepare and wv_rank_labels_prepare blobs; qlab: label word of every query
 *   wv_merge_relbits_map      relbits [G][Q][ceil(kin / 64)], cum [G][Q][nbits + 2] -> ap float32 [Q], nrel int32 [Q] (or NULL),
 *                             need_out as in wv_topk_merge_cum_need
 * relbits_ld / cum_ld: row pitches in uint64 / uint32 units (0 = tight): string and histogram of a (query, shard) may lie side
 * by side in ONE wire buffer, so that a single all_to_all moves both; words of a row that belong to neither are not written.
 * relbits 8-byte, cum 4-byte aligned.
 * wv_hamming_shard_relbits: WV_ENOTSUP outside the windowed kernel's range (shards of more than 32,768 rows, k > 32,639, wider
 * labels); any k inside it: a shard can send the relevance string of its whole ranking (mAP@ALL).
 * wv_merge_relbits_map: WV_ENOTSUP when the k-bit merged string does not fit LDS beside the run boundaries of the G shards
 * (wv_merge_relbits_map_ks_lds_bytes(G, k, nbits) > WV_MERGE_RELBITS_LDS_LIMIT, below); nothing is written, and the caller
 * then merges the lists and runs wv_map_at_k. */
int wv_hamming_shard_relbits(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab,
                             int lwords, uint64_t *relbits, int64_t relbits_ld, uint32_t *cum, int64_t cum_ld, int Q, int64_t N,
                             int nbits, int k, void *stream);
int wv_merge_relbits_map(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q, int kin,
                         int k, int nbits, float *ap, int32_t *nrel, int32_t *need_out, void *stream);

/* Precision and recall by Hamming radius -- what a hash-table lookup within radius r returns -- from ONE pass over the codes,
 * without a [Q][N] distance or relevance matrix and without lists.  Two integer tables per query, uint32 [Q][nbits + 2] each:
 *   cum[q][b]     rows with distance < b (the numbers wv_hamming_hist returns; cum[q][nbits + 1] = N)
 *   cumrel[q][b]  rows with distance < b that share a label bit with the query (label_comparison_fn on multi-hot words;
 *                 cumrel[q][nbits + 1] = all relevant rows; all zero for a query without classes)
 * Within radius r a query finds cum[q][r + 1] rows, cumrel[q][r + 1] of them relevant: the ingredients of pr_curve
 * (precision and recall at every radius 0..nbits, DSCH/_utils.py:469-493) and of get_precision_recall_by_Hamming_Radius
 * (P@H<=2, DSCH/_utils.py:577-594); wvhash/engine/radius_metrics.py turns the tables into those numbers.  Both tables ADD
 * across row shards (counts of disjoint row sets): a database beyond one call's range, or one spread over several GPUs, is
 * the plain sum of the per-shard tables -- one SUM all-reduce, no merge.
 *   prepared / prepared_labels  wv_db_prepare's and wv_rank_labels_prepare's blobs, as for wv_hamming_map_at_k
 *   qlab                        [Q][lwords] label words of the queries, lwords = 1 or 2; nbits <= 128
 * wv_hamming_radius_hist      WV_ENOTSUP outside the windowed kernel (more than 32,768 rows) and for lwords > 2
 * wv_hamming_radius_hist_cpu  host twin (HOST pointers, packed codes and label words, any N): the same integers */
int wv_hamming_radius_hist(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab, int lwords,
                           int Q, int64_t N, int nbits, uint32_t *cum, uint32_t *cumrel, void *stream);
int wv_hamming_radius_hist_cpu(const uint64_t *q, const uint64_t *db, const uint64_t *qlab, const uint64_t *dblab, int lwords, int Q,
                               int64_t N, int nbits, uint32_t *cum, uint32_t *cumrel);

/* Ranking from a stored distance matrix row (same order as wv_hamming_topk).  dist_matrix: any address, any ld_dist >= N. */
int wv_rank_from_dist(const uint8_t *dist_matrix, int64_t ld_dist, int Q, int64_t N, int nbits,
                      int32_t *idx, uint8_t *dist, int k, void *stream);

/* ------------------------------------------------------------------------------------------
 * Average precision of each query over its ranked list.
 * Replaces the per-query body of calculate_maphashing (accuracy_calculator.py:216-229):
 *   gnd = labels share a tag; tgnd = gnd[indices][:topk]; AP = mean_j(j / rank_j) over hits.
 * idx: int32 [Q][k] database rows (as written by wv_hamming_topk); entries < 0 are skipped.
 * qlab [Q][lwords], dblab [N][lwords]: labels packed by wv_pack_bits(mode 1).
 * ap: float32 [Q] (0 when the query has no hit in its list); nrel: int32 [Q] = hits.
 * mAP = sum(ap) / Q  (the reference divides by all queries, :231).
 * ------------------------------------------------------------------------------------------ */
int wv_map_at_k(const int32_t *idx, int Q, int k, const uint64_t *qlab, const uint64_t *dblab,
                int lwords, float *ap, int32_t *nrel, void *stream);

/* The same over the first k entries of longer lists (row pitch ld >= k): mAP@k for several k from ONE ranking at the
 * largest k -- evaluate_multi_k (main/engine/evaluate.py:172-245) re-ranks once per k in the reference. */
int wv_map_at_k_ld(const int32_t *idx, int64_t ld, int Q, int k, const uint64_t *qlab, const uint64_t *dblab,
                   int lwords, float *ap, int32_t *nrel, void *stream);

/* Average precision at SEVERAL cut-offs from one pass (evaluate_all_checkpoints.py --k 5000,117218; evaluate_multi_k's k_list).
 * The list for the largest cut-off has the list for every smaller one as a prefix (the order distance, then row is total) and a
 * list position's thread does not depend on k, so AP@ks[i] is a snapshot of one walk to ks[nk - 1]: column i has the bits the
 * single-k entry point of the same name returns for k = ks[i] (whenever both run the same kernel variant: always for
 * wv_merge_relbits_map_ks, wv_map_at_ks and the 256-thread ranking kernel; one wave per query sums in its own order).
 *   ks    HOST pointer, nk in [1, WV_MAX_CUTOFFS], strictly ascending, 1 <= ks[0], ks[nk - 1] <= N (lists: <= ld); anything
 *         else is WV_EINVAL, answered on the host before any launch
 *   ap    float32 [Q][nk], nrel int32 [Q][nk] or NULL; nothing else is written
 * wv_hamming_map_at_ks    <- wv_hamming_map_at_k: list, window, LDS and relevance bitmap sized by ks[nk - 1]; no list is written
 * wv_merge_relbits_map_ks <- wv_merge_relbits_map: the merged string is assembled for ks[nk - 1], need_out refers to it too;
 *                            the shards send wv_hamming_shard_relbits' string of that prefix
 * wv_map_at_ks            <- wv_map_at_k_ld: the list is read and the labels are gathered once for all cut-offs
 * wv_map_at_ks_cpu        host twin of wv_map_at_ks (HOST pointers), same summation order, bit for bit
 * WV_ENOTSUP when the largest cut-off is outside the fused kernel (wv_hamming_map_at_ks: as wv_hamming_map_at_k) or its merged
 * string does not fit LDS (wv_merge_relbits_map_ks): the caller then runs wv_hamming_topk + wv_map_at_ks. */
#define WV_MAX_CUTOFFS 16
/* dynamic LDS wv_merge_relbits_map_ks and wv_merge_relbits_map (kmax = its k) need for G shards and a largest cut-off kmax
 * (0 for arguments they refuse): their kernels share one LDS layout, sized here.  Either call answers WV_ENOTSUP above
 * WV_MERGE_RELBITS_LDS_LIMIT.  For callers that must know before they exchange anything. */
#define WV_MERGE_RELBITS_LDS_LIMIT (60 * 1024)
size_t wv_merge_relbits_map_ks_lds_bytes(int G, int kmax, int nbits);
int wv_hamming_map_at_ks(const uint64_t *q, const void *prepared, const void *prepared_labels, const uint64_t *qlab, int lwords,
                         int Q, int64_t N, int nbits, const int *ks, int nk, float *ap, int32_t *nrel, void *stream);
int wv_merge_relbits_map_ks(const uint64_t *relbits, int64_t relbits_ld, const uint32_t *cum, int64_t cum_ld, int G, int Q, int kin,
                            const int *ks, int nk, int nbits, float *ap, int32_t *nrel, int32_t *need_out, void *stream);
int wv_map_at_ks(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                 int lwords, float *ap, int32_t *nrel, void *stream);
int wv_map_at_ks_cpu(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                     int lwords, float *ap, int32_t *nrel);

/* NDCG from GRADED relevance -- the number of classes a row shares with the query -- as DSCH/_utils.py:551-574 (NDCG) defines
 * it, without its [Q][N] relevance matrix, its [Q][N] argsort and its per-query sort of all N gains:
 *   rel(q, n) = popcount(qlab[q] & dblab[n]) over the lwords label words (wv_pack_bits mode 1), 0 .. 64 * lwords
 *   gain(r)   = 2^r - 1 as an fp64 value, ldexp(1.0, r) - 1.0: exact for r <= 53 and rounded like the reference's int64 ->
 *               float64 conversion through r = 62.  From r = 63 the reference's int64 2**Rel overflows (2^64 - 1 is -1 there);
 *               above 62 this fp64 value IS the definition and parity with the reference is not claimed.
 *   w[p]      = 1 / log2(p + 2), an fp64 table made once on the host by wv_ndcg_weights (w: HOST pointer, k entries); the
 *               kernel and the twin read the table, neither evaluates a logarithm, neither divides
 *   DCG@k(q)  = sum over p < k of gain(rel(q, idx[q][p])) * w[p]; entries idx < 0 contribute 0, as in wv_map_at_k
 *   IDCG@k(q) = the same sum over the gains of all N rows in descending order, position by position from the histogram:
 *               position p takes the largest r with #{rows with rel >= r} > p, positions past the last row with rel >= 1 add 0
 *   NDCG@k    = (1 / Q) * sum over the queries with IDCG > 0 of DCG / IDCG (wvhash/engine/ndcg.py; the reference divides by
 *               all queries)
 * wv_label_overlap_hist  hist uint32 [Q][64 * lwords + 1], overwritten: hist[q][r] = rows of THIS call that share exactly r
 *                        classes with query q.  One pass over the plain label words, any N >= 1 (N < 2^32): no prepared blob,
 *                        no 32,768-row limit.  The rows of the table ADD across row shards (counts of disjoint row sets), like
 *                        the radius tables above.  No workspace; the zeroing is enqueued on `stream`.
 * wv_ndcg_at_ks          dcg, idcg fp64 [Q][nk] from ranked lists idx int32 [Q][ld] (as wv_hamming_topk / wv_knn_float write
 *                        them) at the cut-offs ks -- wv_map_at_ks' rules: HOST pointer, nk in [1, WV_MAX_CUTOFFS], strictly
 *                        ascending, 1 <= ks[0], ks[nk - 1] <= ld; anything else is WV_EINVAL, answered on the host before any
 *                        launch; the cut-offs travel by value in the kernel arguments.  hist: the table above for the whole
 *                        database; w: DEVICE copy of wv_ndcg_weights' table, >= ks[nk - 1] entries.
 * lwords outside {1, 2} is WV_ENOTSUP.  No workspace, no hidden synchronisation.
 * Summation order, the same in the kernel and in the host twin, so that dcg and idcg agree BIT FOR BIT: position p belongs to
 * thread p % 256, a thread adds its terms in increasing position with fma(gain, w[p], acc), a cut-off c is reduced in the round
 * that holds position c - 1 (threads with p < c contribute their fma, the others their acc): the 64 lanes of a wave in an
 * xor-butterfly, the four waves in index order.  Column i of a multi-cut call has the bits of a call with ks = {ks[i]}.
 * _cpu: host twins (HOST pointers, no stream). */
int wv_label_overlap_hist(const uint64_t *qlab, const uint64_t *dblab, int lwords, int Q, int64_t N, uint32_t *hist, void *stream);
int wv_label_overlap_hist_cpu(const uint64_t *qlab, const uint64_t *dblab, int lwords, int Q, int64_t N, uint32_t *hist);
int wv_ndcg_weights(double *w, int64_t k);
int wv_ndcg_at_ks(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                  int lwords, const uint32_t *hist, const double *w, double *dcg, double *idcg, void *stream);
int wv_ndcg_at_ks_cpu(const int32_t *idx, int64_t ld, int Q, const int *ks, int nk, const uint64_t *qlab, const uint64_t *dblab,
                      int lwords, const uint32_t *hist, const double *w, double *dcg, double *idcg);

/* Running hit counts along each ranked list: hits[q][p] = relevant entries among idx[q][0..p] (uint32 [Q][k]).
 * The ratios of these counts are the secondary retrieval diagnostics of accuracy_calculator.py:131-181
 * (RetrievalRPrecision, RetrievalPrecision(top_k=1), RetrievalPrecisionRecallCurve) and the full-gallery
 * precision/recall curves of calculate_pr_rc_hashing (:235-273).  Same relevance rule as wv_map_at_k. */
int wv_hit_prefix(const int32_t *idx, int Q, int k, const uint64_t *qlab, const uint64_t *dblab,
                  int lwords, uint32_t *hits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Real-valued k-NN (non-binary embeddings).  Replaces get_knn_torch (get_knn.py:60-71):
 *   metric 0: scores = q @ r.T,           top-k largest  (hamming / cosine branch)
 *   metric 1: d = torch.cdist(q, r, p=2), top-k smallest (true L2)
 *   metric 2: the same neighbours with faiss IndexFlatL2's SQUARED distances (get_knn.py:38-39,55)
 * L2 rows are ranked on the squared distance |q|^2 + |r|^2 - 2 q.r (clamped at 0) -- what faiss ranks on, and
 * torch.cdist's order up to the ties the rounding of the root creates; metric 1 takes the root of the k results.
 * Ties are broken by ascending database index.  idx int32 [Q][k], val float32 [Q][k].  Any D >= 1 (rows 16-byte aligned when D % 4 == 0), N <= 2^26,
 * q and db 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define WV_METRIC_IP 0
#define WV_METRIC_L2 1
#define WV_METRIC_L2_SQUARED 2
size_t wv_knn_float_workspace_bytes(int Q, int64_t N, int D, int k);
int wv_knn_float(const float *q, const float *db, int Q, int64_t N, int D, int metric, int k,
                 int32_t *idx, float *val, void *workspace, size_t workspace_bytes, void *stream);
/* Host twin (HOST pointers, no stream, no workspace; csrc/host_knn.cpp): the same indices and values bit for bit --
 * v_mfma_f32_32x32x2_f32 is an fmaf chain (k = 0 before k = 1; tools/mfma_order_test.hip), the twin walks k in the order
 * the kernel feeds it, forms the squared norms in the kernel's lane / butterfly order and ranks on the same keys. */
int wv_knn_float_cpu(const float *q, const float *db, int Q, int64_t N, int D, int metric, int k, int32_t *idx, float *val);

/* The ranking stage of wv_knn_float on scores the caller made: per row of S [Q][N] (dense) the k best columns, smallest
 * first (WV_RANK_DESCENDING: largest first), ties by ascending column -- idx int32 [Q][k] column numbers, val float32
 * [Q][k] their scores (WV_RANK_SQRT: the root of them, for squared distances).  It is the merge of per-shard k-NN lists
 * that faiss' sharded index does on the host (get_knn.py:41-44): the shards' (value, global row) lists laid side by side in
 * shard order rank to exactly the unsharded result (wvhash.parallel.sharded_knn_float).  Host twin: same arguments, host
 * pointers, no workspace / stream. */
#define WV_RANK_DESCENDING 1
#define WV_RANK_SQRT 2
size_t wv_rank_scores_workspace_bytes(int Q, int64_t N, int k);
int wv_rank_scores(const float *S, int Q, int64_t N, int k, int flags, int32_t *idx, float *val, void *workspace,
                   size_t workspace_bytes, void *stream);
int wv_rank_scores_cpu(const float *S, int Q, int64_t N, int k, int flags, int32_t *idx, float *val);

/* ------------------------------------------------------------------------------------------
 * Batch mAP proxy: average precision over the inner-product ranking of REAL-VALUED embeddings, scores, ranking and AP in one
 * launch.  Replaces calculate_maphashing (accuracy_calculator.py:203-231) where its key 0.5 * (nbits - q @ r.T)
 * (calc_hamming_dist :183-186) is taken of tanh values or BN logits: compute_batch_map's self-retrieval mAP of a minibatch
 * (main/engine/batch_map.py, base_update.py:70-73,287-290).  The small problem -- no list wanted, one launch before a
 * .item(); large shapes are wv_knn_float + wv_map_at_k.
 *   q [Q][D], db [N][D] float32, dense; qlab [Q][lwords], dblab [N][lwords]: labels packed by wv_pack_bits(mode 1)
 *   ap float32 [Q], nrel int32 [Q] or NULL.  Every pointer at its natural alignment (D % 4 == 0 and db 16-byte aligned loads
 *   db 16 bytes at a time; any other db four bytes at a time: the same bits)
 * The contract, the same for the kernel and the host twin, bit for bit:
 *   score      s(q, n) = the fp32 value wv_knn_float(metric = WV_METRIC_IP) writes for the pair: one fmaf chain from 0.0f over
 *              k in the order the matrix cores accumulate it (8c + e, 8c + 4 + e for e = 0..3 of every chunk c of eight).
 *   order      descending score, ties by ascending row, on wv_knn_float's order-preserving 32-bit key: -0 equals +0; a NaN
 *              with the sign bit clear ranks before +inf (first), a NaN with the sign bit set after -inf (last), NaNs of one
 *              sign among themselves by payload.  The reference's key 0.5f * (D - s) is a non-increasing function of s and
 *              its argsort is not stable: this order is one of the orders the reference can itself produce.
 *   relevance  (qlab[q] & dblab[row]) != 0 over the lwords words.
 *   AP         over the first k positions with the arithmetic and the summation order of wv_map_at_k: ap and nrel equal, bit
 *              for bit, wv_map_at_k applied to the idx wv_knn_float(IP, k) returns for the same inputs.  A query without a
 *              hit: ap = 0, nrel = 0.
 * Arguments are checked on the host before any launch, the message names the argument: WV_EINVAL for a null pointer (nrel
 * excepted), Q < 0, N < 1, D < 1, k outside [1, N], lwords outside {1, 2}; WV_ENOTSUP for N > WV_IP_MAP_ROWS_MAX (the ranked
 * list of a query lives in one workgroup's LDS) or D > 512 (the staged query row), the message names the limit.  Q = 0 writes
 * nothing and returns 0.  No workspace, asynchronous on `stream`, no hidden synchronisation.
 * _cpu: host twin (HOST pointers, no stream; csrc/host_ip_map.cpp): the composition of wv_knn_float_cpu and wv_map_at_k_cpu the
 * contract is defined by, under the same argument rules.
 * ------------------------------------------------------------------------------------------ */
#define WV_IP_MAP_ROWS_MAX 2048
int wv_ip_map_at_k(const float *q, const float *db, int Q, int64_t N, int D, const uint64_t *qlab, const uint64_t *dblab,
                   int lwords, int k, float *ap, int32_t *nrel, void *stream);
int wv_ip_map_at_k_cpu(const float *q, const float *db, int Q, int64_t N, int D, const uint64_t *qlab, const uint64_t *dblab,
                       int lwords, int k, float *ap, int32_t *nrel);

/* ------------------------------------------------------------------------------------------
 * Band-attention pooling head + hashing tail (eval mode).
 * Replaces CrossAttentionBottleneckHeadAdvanced.forward (multi_dino_attention.py:1111-1141;
 * same core in ...Head :1030-1062, ...Pooled :568-599, ...Decoupled :448-481) and
 * SharedDinoHashing's tail hash_fc -> BatchNorm1d(eval) -> sign (:829-833).
 * All weights row-major fp32 exactly as in the module's state_dict.
 * ------------------------------------------------------------------------------------------ */
typedef struct wv_head_params {
    int embed_dim;   /* E (multiple of 32; 384 for ViT-S) */
    int num_heads;   /* E % num_heads == 0 */
    int num_queries; /* Nq */
    int num_tokens;  /* S = 4 band tokens */
    int pool_mean;   /* 0: concat read-out (Nq*E -> E), 1: mean read-out (E -> E) */
    const float *q_eff;      /* [Nq][E] effective query tokens (after optional normalise*scale) */
    const float *in_proj_w;  /* [3E][E] */
    const float *in_proj_b;  /* [3E] */
    const float *attn_out_w; /* [E][E] */
    const float *attn_out_b; /* [E] */
    const float *norm1_w, *norm1_b; /* [E] */
    const float *mlp0_w;     /* [4E][E] */
    const float *mlp0_b;     /* [4E] */
    const float *mlp2_w;     /* [E][4E] */
    const float *mlp2_b;     /* [E] */
    const float *out_w;      /* [E][Nq*E] or [E][E] */
    const float *out_b;      /* [E] */
    const float *norm2_w, *norm2_b; /* [E] */
    float ln_eps;
    /* optional: [Nq][E] projected queries  q_eff @ Wq^T + bq  made once by wv_band_attn_qproj (the query tokens are
     * parameters: in eval mode their projection does not change from call to call); NULL = computed in every call */
    const float *q_proj;
    /* optional: the blob wv_band_attn_prepare wrote (projected queries + the weights of every product up to the MLP
     * output in MFMA-fragment order, with the K projection folded into the queries).  When set, and the configuration
     * has a fused kernel (wv_band_attn_prepared_bytes != 0), everything before the read-out product runs as ONE
     * launch (csrc/head_front.hip) and q_proj is not needed.  It is a snapshot of in_proj_w, q_eff, attn_out_w, mlp0_w,
     * mlp2_w: make it again whenever one of them changes.  NULL = separate launches (any configuration). */
    const void *prepared;
} wv_head_params;

size_t wv_band_attn_pool_workspace_bytes(const wv_head_params *p, int B);
/* q_proj_out float32 [Nq][E] = q_eff @ in_proj_w[0:E]^T + in_proj_b[0:E] (the Q third of nn.MultiheadAttention's packed
 * in-projection, multi_dino_attention.py:1081,1128) */
int wv_band_attn_qproj(const wv_head_params *p, float *q_proj_out, void *stream);
/* Size of the prepared blob for this configuration; 0 = no fused kernel (E = 384, 4 band tokens and 4 or 8 queries
 * have one), use the separate-launch path.  wv_band_attn_prepare fills `prepared_out` (device memory of that size) on
 * `stream`; p->q_proj and p->prepared are ignored by it.  The weights are parameters (multi_dino_attention.py:1064-1109):
 * in eval mode the blob is made once per parameter update, like q_proj. */
size_t wv_band_attn_prepared_bytes(const wv_head_params *p);
int wv_band_attn_prepare(const wv_head_params *p, void *prepared_out, void *stream);
/* feats: [S][B][E] (band-major, the layout cls_tokens.chunk(4) has at :824) -> out [B][E] */
int wv_band_attn_pool(const wv_head_params *p, const float *feats, int B, float *out,
                      void *workspace, size_t workspace_bytes, void *stream);

/* logits = fused @ hash_w.T (+ hash_b); BN(eval); codes = sign(logits) as fp32 and bit-packed.
 * Any of logits_out / codes_out / packed_out may be NULL.  bn_* NULL = no BatchNorm.
 *   - codes is +1, -1, or 0.0 for a logit of exactly zero; a NaN logit is passed through as NaN.
 *   - the packed bit is logit > 0, so a zero and a NaN logit both pack as 0 (wv_pack_bits in mode 0 flags those codes).
 *   - packed_out is [B][ceil(nbits / 64)] words; the pad bits of the last word above nbits are 0.
 *   - E % 4 == 0, E >= 4, 4 E bytes <= 48 KB, nbits >= 1 (WV_EINVAL otherwise, checked before any launch); B = 0 writes nothing. */
int wv_hash_tail(const float *fused, int B, int E, const float *hash_w, const float *hash_b,
                 const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var,
                 float bn_eps, int nbits, float *logits_out, float *codes_out,
                 uint64_t *packed_out, void *stream);

/* Host twins of the two entry points above (HOST pointers everywhere, incl. the members of wv_head_params; q_proj and
 * prepared are ignored; no stream, no workspace; csrc/host_head.cpp) for a model whose tensors live on the host.  fp32 with
 * a machine-independent summation order (eight interleaved fmaf chains, one fixed tree); they agree with the kernels to
 * fp32 rounding (both are held to the reference-made golden vectors with the same tolerance), the codes wherever the
 * logit is not within that of zero.  wv_hash_tail_cpu follows the rules of wv_hash_tail for zero and NaN logits, the packed bit
 * and the pad bits; it needs E % 8 == 0 (the kernels: E % 4 == 0) and returns WV_EINVAL otherwise. */
int wv_band_attn_pool_cpu(const wv_head_params *p, const float *feats, int B, float *out);
int wv_hash_tail_cpu(const float *fused, int B, int E, const float *hash_w, const float *hash_b, const float *bn_w,
                     const float *bn_b, const float *bn_mean, const float *bn_var, float bn_eps, int nbits,
                     float *logits_out, float *codes_out, uint64_t *packed_out);

/* ------------------------------------------------------------------------------------------
 * Opt-in bf16 matrix-core path of the same head: what the reference computes when its forward runs under
 * torch.autocast(dtype=torch.bfloat16) (main/models/net.py:475, config/model/...: with_autocast: True).  fp32 stays the
 * default; nothing above changes.  Numerical contract, the same for the kernels and the host twin:
 *   - both operands of every dense weight product (K | V in-projection, attention out-projection, mlp.0, mlp.2, read-out) are
 *     bf16, rounded to nearest even; the weights once, by wv_band_attn_bf16_prepare, from the fp32 state_dict tensors `p`
 *     points to; activations where they are read as an operand;
 *   - every product accumulates in fp32 (v_mfma_f32_32x32x16_bf16); the query projection, biases, residual adds, the softmax
 *     over the band tokens, both LayerNorms and GELU are fp32; out is fp32 [B][E];
 *   - feats: [S][B][E] as fp32 (WV_DT_F32) or bf16 (WV_DT_BF16), read in place -- no converted copy is made.
 * The hashing tail stays fp32: wv_hash_tail takes this path's fp32 output as it takes the fp32 head's (the product is
 * nbits x E, e.g. 64 x 384, and not worth a second kernel).
 * Covers every configuration wv_band_attn_pool accepts with E % 32 == 0.  prepared blob (device memory, made again whenever
 * q_eff, in_proj_*, attn_out_w, mlp0_w, mlp2_w or out_w change): the projected queries and the bf16 copies of the five weight
 * matrices; p->q_proj and p->prepared are ignored.  wv_band_attn_bf16_prepared_bytes returns 0 for a configuration the
 * path does not cover.  Errors: WV_EINVAL for E % 32 != 0, a null blob or an unknown feat_dtype (checked on the host before
 * anything is launched), WV_ENOTSUP for a shape outside the kernels -- never a silent fp32 run.
 * Host twin (HOST pointers, no blob: it rounds the weights itself): wv_band_attn_pool_cpu with the operands rounded as above
 * and nothing else -- same fixed summation order, no rounding of intermediates between products.
 * ------------------------------------------------------------------------------------------ */
size_t wv_band_attn_bf16_prepared_bytes(const wv_head_params *p);
int wv_band_attn_bf16_prepare(const wv_head_params *p, void *prepared_out, void *stream);
size_t wv_band_attn_pool_bf16_workspace_bytes(const wv_head_params *p, int B);
int wv_band_attn_pool_bf16(const wv_head_params *p, const void *prepared_bf16, const void *feats, int feat_dtype, int B,
                           float *out, void *workspace, size_t workspace_bytes, void *stream);
int wv_band_attn_pool_bf16_cpu(const wv_head_params *p, const void *feats, int feat_dtype, int B, float *out);

/* ------------------------------------------------------------------------------------------
 * Attention maps of the head: what its nn.MultiheadAttention submodule returns for the call the forward makes
 * (attn(query = q_eff broadcast over the batch, key = value = the band tokens)), as outputs of their own.  wv_band_attn_pool
 * keeps these values in LDS; this is the diagnostic path for forward hooks on `head.attn` and for studies of the attention.
 * Any subset of the four outputs, at least one:
 *   probs       [B][H][Nq][S]  softmax over the S band tokens, per head (average_attn_weights=False)
 *   probs_mean  [B][Nq][S]     its mean over the H heads, summed in head order (the module's default output[1])
 *   scores      [B][H][Nq][S]  what the softmax is taken of: (q Wq^T + bq) . (k Wk^T + bk) / sqrt(E / H)
 *   attn_out    [B][Nq][E]     out_proj(context) + bias (output[0])
 * feats: the band tokens, [S][B][E] (WV_TOKENS_SBE: what wv_band_attn_pool takes) or [B][S][E] (WV_TOKENS_BSE:
 * torch.stack(kv_list, 1), the module's batch_first key), fp32, read in place.
 * Of `p` only embed_dim, num_heads, num_queries, num_tokens, q_eff, in_proj_w, in_proj_b, attn_out_w, attn_out_b and the
 * optional q_proj are read (ranges as for wv_band_attn_pool); every other pointer may be NULL and `prepared` is ignored.
 * Always fp32 arithmetic, that of wv_band_attn_pool's separate launches in the same order (fmaf chain over the head
 * dimension, x scale, max-subtracted expf, sum over the tokens in index order, one division); V is projected only when
 * attn_out is asked for.  Workspace: device memory of wv_band_attn_maps_workspace_bytes(p, B) bytes (enough for any subset).
 * B == 0: WV_OK, nothing touched.  WV_EINVAL: no output asked for, an unknown layout, a workspace shorter than that (the text
 * names the need), parameters out of range; WV_ENOTSUP: a shape wv_band_attn_pool refuses for its LDS need.  All answered on
 * the host before anything is launched.  No hidden synchronisation.
 * Host twin (HOST pointers, no workspace, no stream, q_proj ignored): the same outputs with the summation orders above and
 * the twins' eight-chain products; agrees with the kernel to fp32 rounding, not bit for bit.
 * ------------------------------------------------------------------------------------------ */
enum { WV_TOKENS_SBE = 0, WV_TOKENS_BSE = 1 };
size_t wv_band_attn_maps_workspace_bytes(const wv_head_params *p, int B);
int wv_band_attn_maps(const wv_head_params *p, const float *feats, int layout, int B, float *probs, float *probs_mean,
                      float *scores, float *attn_out, void *workspace, size_t workspace_bytes, void *stream);
int wv_band_attn_maps_cpu(const wv_head_params *p, const float *feats, int layout, int B, float *probs, float *probs_mean,
                          float *scores, float *attn_out);

/* ------------------------------------------------------------------------------------------
 * Image sizing: crop -> resample -> window / zero pad -> mirror, for a RAGGED batch of 3-channel uint8 HWC images in one
 * launch -- what stands in front of the wavelet transform in the reference's YAML pipelines (config/transform/basic_swt.yaml:
 * Resize -> CenterCrop | RandomResizedCrop -> RandomHorizontalFlip on PIL images inside DataLoader workers) and the BICUBIC
 * fix_size of BaseWaveletTransform (custom_transforms.py:132-141).  The resample is Pillow's 8-bit ImagingResample restated
 * (csrc/image_size.hpp): horizontal pass, then vertical pass, 22-bit fixed-point coefficients, uint8 intermediate; an axis
 * whose length does not change is not resampled.  Bit-identical to Image.resize of Pillow 12 for both filters; the device
 * entry point and the host twin agree byte for byte (the coefficient routine is one function compiled for both).
 * One wv_size_stage is one step of one image:
 *   1. the integer rectangle crop_* of the source is a new image (bounds clamp at ITS edge, as img.crop(box).resize(...));
 *   2. it is resampled to res_h x res_w with `filter`;
 *   3. the out_h x out_w window at (win_y, win_x) of the resampled image is written to dst; the window may hang over any edge:
 *      pixels outside [0, res) are 0 (torchvision's CenterCrop zero-pads an image smaller than the crop);
 *   4. flip != 0 mirrors the written window left-right.
 * src / dst: base pointers of two byte buffers; an image lies at src + src_offset with row pitch src_row_bytes (dst likewise).
 * A pipeline with two resamples is two stages (two launches, the first writing an intermediate ragged buffer).
 * wv_image_size        stages: DEVICE array of n descriptors.  max_out_h / max_out_w / max_ksize: maxima over the n stages of
 *                      out_h, out_w and the tap count min(ceil(S * max(crop / res, 1)) * 2 + 1, crop) of either axis (S = 1
 *                      bilinear, 2 bicubic; 1 for an unchanged axis) -- they size the grid and the LDS, the kernel reads everything
 *                      else from the descriptors.  No workspace, no table, no copy, no hidden synchronisation.  The descriptors
 *                      are device memory: the entry point cannot check them; the caller runs wv_image_size_check on its host
 *                      copy before the upload.  Maxima smaller than the truth leave pixels unwritten, never write elsewhere.
 * wv_image_size_cpu    host twin (HOST pointers); runs wv_image_size_check itself.
 * wv_image_size_check  the one argument check (HOST descriptors): WV_EINVAL for values that describe no image (a side < 1, a
 *                      crop outside the source, a row pitch shorter than the row, a negative offset, an unknown filter,
 *                      destinations of two stages that overlap), WV_ENOTSUP for images outside the kernel's limits (a side above
 *                      16384, a window origin beyond +-16384, a down-scale above 64 on an axis of more than 257 samples -- 257 taps
 *                      per coefficient row is what the limit protects, and a row has no more taps than its axis has samples);
 *                      the message names the field.
 * ------------------------------------------------------------------------------------------ */
#define WV_RESAMPLE_BILINEAR 2 /* PIL's enum values */
#define WV_RESAMPLE_BICUBIC 3
typedef struct wv_size_stage {
    int64_t src_offset, dst_offset;         /* bytes from `src` / `dst` to the image's first pixel */
    int32_t src_h, src_w, src_row_bytes;
    int32_t crop_y, crop_x, crop_h, crop_w; /* integer rectangle that is resampled */
    int32_t res_h, res_w;                   /* size the rectangle is resampled to */
    int32_t win_y, win_x, out_h, out_w;     /* window of the resampled image that is written */
    int32_t dst_row_bytes, filter, flip;
} wv_size_stage;
int wv_image_size(const uint8_t *src, uint8_t *dst, const wv_size_stage *stages, int n, int max_out_h, int max_out_w,
                  int max_ksize, void *stream);
int wv_image_size_cpu(const uint8_t *src, uint8_t *dst, const wv_size_stage *stages, int n);
int wv_image_size_check(const wv_size_stage *stages, int n);

/* ------------------------------------------------------------------------------------------
 * Colour jitter: brightness, contrast and saturation in a per-image order, IN PLACE on a ragged batch of 3-channel uint8 HWC
 * images inside one byte buffer -- torchvision's ColorJitter on PIL input (config/transform/voc_swt.yaml, cub_swt.yaml:
 * brightness = contrast = saturation = 0.25, hue 0), which is Pillow's ImageEnhance.  Restated in csrc/colour.hpp; bit-identical
 * to ImageEnhance of Pillow 12, and the device entry point and the host twin agree byte for byte.
 * Every operation is Image.blend(degenerate, image, factor): byte = (uint8)clamp((float)d + f * (float)(x - d), 0, 255), one
 * fp32 multiply and one fp32 add, truncated; d = 0 (brightness), L of the pixel (saturation), or int(mean(L) + 0.5) of the
 * whole image AS IT IS WHEN CONTRAST RUNS (contrast); L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16.  Hue is not
 * implemented.
 * One wv_colour_ops is one image: it lies at img + offset, h rows of w pixels, row pitch row_bytes; kind[0 .. n_ops) and
 * factor[0 .. n_ops) are its operations in the order they run (n_ops = 0: the image is left alone).
 * wv_colour_jitter                 ops: DEVICE array of n descriptors.  max_h / max_w: maxima of h and w over them (they size
 *                                  the grid; smaller than the truth leaves pixels unchanged, never writes elsewhere).
 *                                  Two launches: the L sums of the images whose chain has contrast (64-bit integers in
 *                                  `workspace`, which the entry point clears on the stream), then the chain.  Only bytes of
 *                                  the images' rows are written; gaps between images and row padding are never touched.  No
 *                                  hidden synchronisation.  The descriptors are device memory: the caller runs
 *                                  wv_colour_jitter_check on its host copy before the upload.
 * wv_colour_jitter_workspace_bytes the n 64-bit sums; a shorter workspace is WV_ENOMEM.
 * wv_colour_jitter_cpu             host twin (HOST pointers); runs wv_colour_jitter_check itself.
 * wv_colour_jitter_check           the one argument check (HOST descriptors): WV_EINVAL for a side < 1, a row pitch shorter
 *                                  than the row, a negative offset, an unknown kind, a kind listed twice, n_ops outside 0..3, a
 *                                  factor that is negative or not finite, images of two descriptors that overlap; WV_ENOTSUP
 *                                  for a side above 16384; the message names the field.
 * ------------------------------------------------------------------------------------------ */
#define WV_COLOUR_BRIGHTNESS 0
#define WV_COLOUR_CONTRAST 1
#define WV_COLOUR_SATURATION 2
typedef struct wv_colour_ops {
    int64_t offset; /* bytes from `img` to the image's first pixel */
    int32_t h, w, row_bytes;
    int32_t n_ops;
    int32_t kind[3]; /* WV_COLOUR_*, in the order the operations run */
    float factor[3];
} wv_colour_ops;
size_t wv_colour_jitter_workspace_bytes(int n);
int wv_colour_jitter(uint8_t *img, const wv_colour_ops *ops, int n, int max_h, int max_w, void *workspace,
                     size_t workspace_bytes, void *stream);
int wv_colour_jitter_cpu(uint8_t *img, const wv_colour_ops *ops, int n);
int wv_colour_jitter_check(const wv_colour_ops *ops, int n);

/* ------------------------------------------------------------------------------------------
 * Grouped LayerNorm: MultiDomainLayerNorm.forward of main/models/multi_dino_attention.py:922-929 -- x.chunk(G, 0), one
 * nn.LayerNorm per chunk, torch.cat -- as one pass.  Restated in csrc/group_layernorm.hpp.
 * x, out: [N][T][E], tightly packed, WV_DT_F32 or WV_DT_BF16 each (any pairing); out must not be x.  gamma, beta: [G][E] fp32.
 * Sequence n takes gamma / beta of group n / ceil(N / G): torch.chunk, including N % G != 0 and N < G (fewer groups in use).
 * Per row, in fp32: mean, biased variance of the centred values, 1 / sqrt(var + eps), ((x - mean) * rstd) * gamma + beta;
 * bf16 is widened on load and rounded to nearest even on store.  Any E >= 1; E % 4 == 0 moves 16 bytes (fp32) or 8 bytes
 * (bf16) per lane when x, out, gamma and beta are aligned to it, element by element otherwise: the same bits.  N * T == 0: WV_OK,
 * nothing touched (pointers may be NULL).
 * wv_group_layernorm       DEVICE pointers; one launch on `stream`, no workspace, no hidden synchronisation.
 * wv_group_layernorm_cpu   host twin (HOST pointers): the kernel's order of sums replayed, equal to it bit for bit.
 * wv_group_layernorm_check the argument check both run first: WV_EINVAL for an unknown dtype, N < 0, T < 0, E < 1, G < 1;
 *                          WV_ENOTSUP for more than 4 * (2^31 - 1) rows.  Both entry points then refuse (WV_EINVAL) a NULL
 *                          x / out / gamma / beta and out == x; every message names the argument.
 * ------------------------------------------------------------------------------------------ */
int wv_group_layernorm_check(int x_dtype, int out_dtype, int64_t N, int64_t T, int E, int G);
int wv_group_layernorm(const void *x, int x_dtype, void *out, int out_dtype, int64_t N, int64_t T, int E, int G,
                       const float *gamma, const float *beta, float eps, void *stream);
int wv_group_layernorm_cpu(const void *x, int x_dtype, void *out, int out_dtype, int64_t N, int64_t T, int E, int G,
                           const float *gamma, const float *beta, float eps);

/* ------------------------------------------------------------------------------------------
 * Pairwise hashing losses: value AND gradient w.r.t. the embeddings of SCHLoss.forward (main/losses/dsch.py:31-59) and
 * HashNetLoss.forward (main/losses/hashnet_loss.py:49-66) -- in the reference about 25 elementwise, boolean-index and reduction
 * ops on [B, B] tensors, forward and again backward.  Here two launches; no [B, B] matrix reaches memory.
 *   e      [B][D] float32, dense: the embeddings
 *   labels [B][lwords]: multi-hot labels packed by wv_pack_bits(mode 1)
 *   out    float32 [3]: the loss and its two parts (SCH: loss1, loss2; HashNet: the means over the pairs that share a label and
 *          over those that do not)
 *   grad   float32 [B][D]: d loss / d e, or NULL -- then that part of the work is skipped and `out` has the same bits.
 * With n_i = |L_i|, c_ij = |L_i & L_j|, u = tanh(pre_scale * e) (apply_tanh != 0) or pre_scale * e, G = u u^T:
 *   WV_PAIR_LOSS_SCH      k = nbits; S = c / sqrt(n_i n_j) (0 where n_i n_j = 0); same: c = n_i = n_j > 0; disjoint: c = 0;
 *                         lambda = (1 - S) k / 2; lambda_l = max(lambda - 3, 0), k / 2 where disjoint; W_l = 0 | beta | 1 and
 *                         W_u = alpha | 0 | 1 for same | disjoint | other; H = (k - G) / 2;
 *                         loss = |relu(lambda_l - H) W_l|_F / B^2 + |relu(H - lambda) W_u|_F / B^2, diagonal included.  A part
 *                         whose norm is 0 has gradient 0 (torch.norm's backward), never NaN.  `same` is the exact set relation,
 *                         not the reference's fp32 test S == 1.
 *   WV_PAIR_LOSS_HASHNET  P = c > 0; dp = alpha G; t = softplus(dp) - P dp; S1 = #P, S0 = B^2 - S1;
 *                         loss = sum_P t / S1 + sum_notP t / S0, an empty class contributing nothing.  nbits, beta unused.
 * fp32 arithmetic (G by fmaf), the two global sums in double.  No floating-point atomics: the same call gives the same bits.
 * Everything is enqueued on `stream`; no hidden synchronisation.
 * workspace: device memory of wv_pair_loss_workspace_bytes(B, D) bytes (two [B][D] fp32 sums + one record per 8 rows), 16-byte
 * aligned (WV_EINVAL otherwise), written before it is read.  e, out, grad: 4-byte aligned.
 * Arguments are checked on the host before any pointer is read: WV_EINVAL for a null pointer (grad excepted), B < 1, D < 1,
 * lwords outside {1, 2}, an unknown kind, pre_scale <= 0, a workspace shorter than the query says; WV_ENOTSUP for
 * B > WV_PAIR_LOSS_ROWS_MAX or D > 512; the message names the argument.
 * _cpu: host twin (HOST pointers, no workspace, no stream; csrc/host_pair_loss.cpp) under the same rules, the same per-pair
 * code (csrc/pair_loss.hpp); it agrees with the kernel to fp32 rounding, not bit for bit (device tanh / exp / log1p).
 * ------------------------------------------------------------------------------------------ */
#define WV_PAIR_LOSS_SCH 0
#define WV_PAIR_LOSS_HASHNET 1
#define WV_PAIR_LOSS_ROWS_MAX 2048
typedef struct wv_pair_loss_params {
    int kind;        /* WV_PAIR_LOSS_* */
    int apply_tanh;  /* u = tanh(pre_scale * e) instead of pre_scale * e */
    float pre_scale; /* > 0; HashNet's continuation scale, 1 for SCH */
    float nbits;     /* SCH: k */
    float alpha;     /* SCH: W_u of `same` pairs; HashNet: the factor of G inside the sigmoid */
    float beta;      /* SCH: W_l of `disjoint` pairs */
} wv_pair_loss_params;
size_t wv_pair_loss_workspace_bytes(int B, int D);
int wv_pair_loss(const float *e, const uint64_t *labels, int lwords, int B, int D, const struct wv_pair_loss_params *p,
                 float *out, float *grad, void *workspace, size_t workspace_bytes, void *stream);
int wv_pair_loss_cpu(const float *e, const uint64_t *labels, int lwords, int B, int D, const struct wv_pair_loss_params *p,
                     float *out, float *grad);

/* ------------------------------------------------------------------------------------------
 * Rank-approximation AP losses: SmoothAP and SupAP (main/losses/smooth_rank_ap.py), the AP of every query row AND its
 * gradient w.r.t. that row's scores.  The reference materialises S[q,j] - S[q,i] as a [B, B, B] tensor, rewrites it with
 * boolean-mask assignments and keeps all of it for autograd (quick_forward), or loops over the B queries in Python
 * (general_forward).  Here nothing of size B x M x M exists: one workgroup per query row, the row in LDS.
 *   scores [B][M] float32, dense
 *   target [B][M] float32 holding 0 / 1 (any non-zero value counts as 1)
 *   ap     float32 [B]: AP_q
 *   grad   float32 [B][M]: d AP_q / d scores[q][.], or NULL -- then that part of the work is skipped and `ap` has the same
 *          bits.  Row q of the gradient depends on row q of the scores only.
 * For query row q:  P = { i : T[q,i] = 1 },  n = |P|,  d_ij = S[q,j] - S[q,i]  (i in P, all j),
 *   sigma(x) = 1 / (1 + exp(clamp(-x / tau, -50, 50))),  derivative sigma (1 - sigma) / tau inside the clamp, 0 outside.
 *   WV_RANK_AP_SMOOTH  R_ij = sigma(d_ij); the pair's target bit is ignored.
 *   WV_RANK_AP_SUP     where tgt_ij: R = [d >= 0], derivative 0;  elsewhere  d > delta: R = rho (d - delta) + offset, derivative
 *                      rho;  0 < d <= delta: R = start + sigma(d);  d <= 0: R = sigma(d).  `offset` is a number: the caller
 *                      resolves the reference's offset=None to start + sigma(delta).
 *   WV_RANK_AP_GENERAL any [B][M]:      tgt_ij = T[q,j],  w_ij = T[q,j]
 *   WV_RANK_AP_QUICK   B = M required:  tgt_ij = LM[i,j] and T[q,j] with LM = (T T^t > 0),  w_ij = T[i,j] (row i, not row q)
 *   rk_i = 1 + sum_{j != i} R_ij,  prk_i = 1 + sum_{j != i} R_ij w_ij,  AP_q = (1 / n) sum_{i in P} prk_i / rk_i.
 *   With f_i = prk_i / rk_i and g_ij = (w_ij - f_i) / (rk_i n) R'_ij (j != i):  grad[q][j] += g_ij,  grad[q][i] -= g_ij.
 * The quick form equals the reference's quick_forward for targets with T[i,i] = 1 (a label matrix of non-empty rows has
 * them); for T[i,i] = 0 the reference subtracts R_ii from prk_i, which this entry point does not.
 * A row without a positive gives ap 0 and grad 0 (the reference: 0 / 0 = NaN).
 * fp32 arithmetic; every sum has one fixed order, no floating-point atomics: the same call gives the same bits.
 * Two launches for the general form (bit-packing of T; the rows), three for the quick form (the bit rows of LM between
 * them), all on `stream`; no hidden synchronisation.
 * workspace: device memory of wv_rank_ap_workspace_bytes(B, M, form) bytes: the bit rows of T, [B][ceil(M / 64)] 64-bit
 * words, and for the quick form as many for LM; 16-byte aligned (WV_EINVAL otherwise), written before it is read.  scores,
 * target, ap, grad: 4-byte aligned.
 * Arguments are checked on the host before any pointer is read: WV_EINVAL for a null pointer (grad excepted), B < 1, M < 1, an
 * unknown kind or form, the quick form with B != M, tau not > 0, a workspace shorter than the query says; WV_ENOTSUP for
 * B or M above WV_RANK_AP_COLS_MAX (a row, its bit mask, its positives' list and their records live in one workgroup's LDS).
 * _cpu: host twin (HOST pointers, no workspace, no stream; csrc/host_rank_ap.cpp) under the same rules and the same
 * per-pair code (csrc/rank_ap.hpp); it agrees with the kernel to fp32 rounding, not bit for bit (device exp, sum order).
 * ------------------------------------------------------------------------------------------ */
#define WV_RANK_AP_SMOOTH 0
#define WV_RANK_AP_SUP 1
#define WV_RANK_AP_QUICK 0
#define WV_RANK_AP_GENERAL 1
#define WV_RANK_AP_COLS_MAX 4096
typedef struct wv_rank_ap_params {
    int kind;     /* WV_RANK_AP_SMOOTH | WV_RANK_AP_SUP */
    int form;     /* WV_RANK_AP_QUICK | WV_RANK_AP_GENERAL */
    float tau;    /* > 0: the sigmoid's temperature */
    float rho;    /* SUP: slope beyond delta */
    float offset; /* SUP: value at d = delta+ */
    float delta;  /* SUP: where the linear part begins (the reference's delta=None: 0) */
    float start;  /* SUP: added to the sigmoid on 0 < d <= delta */
} wv_rank_ap_params;
size_t wv_rank_ap_workspace_bytes(int B, int M, int form);
int wv_rank_ap(const float *scores, const float *target, int B, int M, const struct wv_rank_ap_params *p, float *ap,
               float *grad, void *workspace, size_t workspace_bytes, void *stream);
int wv_rank_ap_cpu(const float *scores, const float *target, int B, int M, const struct wv_rank_ap_params *p, float *ap,
                   float *grad);

#ifdef __cplusplus
}
#endif
#endif /* WVHASH_H */
