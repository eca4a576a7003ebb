// Argument rules the head's device entry points (head.hpp) and the attention-map host twin (host_head.cpp) share.  Plain
// C++: no HIP header, so the host twins can include it.
#pragma once
#include <stdio.h>

#include "../../include/wvhash.h"

namespace wv {

// The attention part of wv_head_params -- shapes, query tokens, packed in-projection, attention out-projection: all that
// wv_band_attn_maps reads, and the first half of what wv_band_attn_pool checks.  Returns WV_OK, or the refusal's code with
// its text in why.  what: the entry point's name in that text.
inline int head_attn_args_refusal(const wv_head_params *p, int B, const char *what, char *why, size_t nwhy)
{
#define WV_ARGS_REFUSE(...) (snprintf(why, nwhy, __VA_ARGS__), WV_EINVAL)
    if (!p) return WV_ARGS_REFUSE("%s: null params", what);
    const int E = p->embed_dim;
    if (B < 0) return WV_ARGS_REFUSE("%s: B=%d", what, B);
    if (!(E >= 8 && E % 8 == 0)) return WV_ARGS_REFUSE("%s: embed_dim=%d must be a multiple of 8", what, E);
    if (!(p->num_heads >= 1 && E % p->num_heads == 0))
        return WV_ARGS_REFUSE("%s: embed_dim %d not divisible by num_heads %d", what, E, p->num_heads);
    if (!(p->num_queries >= 1 && p->num_queries <= 64)) return WV_ARGS_REFUSE("%s: num_queries=%d", what, p->num_queries);
    if (!(p->num_tokens >= 1 && p->num_tokens <= 64)) return WV_ARGS_REFUSE("%s: num_tokens=%d", what, p->num_tokens);
    if (!(p->q_eff && p->in_proj_w && p->in_proj_b && p->attn_out_w && p->attn_out_b))
        return WV_ARGS_REFUSE("%s: null weight pointer", what);
#undef WV_ARGS_REFUSE
    return WV_OK;
}

// what the attention kernels keep in LDS per sample: kv[S][2E + 4] | q[Nq][E] | P[Nq][heads][S]
inline size_t head_attn_lds_bytes(const wv_head_params *p)
{
    const size_t E = p->embed_dim, Nq = p->num_queries, S = p->num_tokens;
    return (S * (2 * E + 4) + Nq * E + Nq * p->num_heads * S) * sizeof(float);
}

}  // namespace wv
