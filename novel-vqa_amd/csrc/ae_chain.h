// ae_chain.h -- the integer rules of an auto-encoder step (ae.hip), each written once.  Plain C++, no HIP header: the kernels, the
// host paths and the g++ checker tests/shim/ae_chain_check.cc compile the same text.
//
// One step is a chain of te encoder steps, then nd = tmax + 1 decoder steps (tmax = the last column of the batch with a non-null
// token; chain step q = te + s is decoder step s).  Tokens are 1-based, 0 = null and is fed as 1, START = END = V + 1.
//   AE1 (te = tmax)      q < te: lookup of tok[:, q];  q = te + s: START, then lookup of tok[:, s-1]
//   AE2 (te = tmax + 2)  q = 0, 1: the image row [B x E], START;  q in [2, te): lookup of tok[:, q-2];  the decoder as above
//   AE2_WP, AE1_WP       as AE2 / AE1, but the encoder reads enc_tokens (te = 2 + tmax(enc_tokens) / tmax(enc_tokens); the null
//                        sentence has tmax 0), the decoder and the criterion read tokens
#pragma once
#include <stdint.h>

#include <vector>

#include "nvqa_rng.h"

namespace nvqa {

#define NVQA_AE_LK_CHUNK 16 // rows of one token that the lookup gradient sums in one workgroup (ae.hip k_ae_lk_part)

// AE2: the image row and START in front of the encoder's tokens (NVQA_ARCH_AE2, _AE2_WP); BRIDGE: the bridge between the LSTMs
// (NVQA_ARCH_AE1_WP); ENC: the encoder reads a token stream of its own (both weak-paired archs)
enum { AE_CHAIN_AE2 = 1, AE_CHAIN_BRIDGE = 2, AE_CHAIN_ENC = 4 };

struct AeChain { int B, D, V, te, nd, flags; }; // rows, seq_length, vocabulary; encoder, decoder steps; AE_CHAIN_*.  A kernel argument

// te.  skip (AE1_WP): the caller gave the encoder's final state instead of its tokens
NVQA_HD int encoder_steps(int flags, int tmax, int tmax_enc, bool skip)
{
    return (flags & AE_CHAIN_AE2 ? 2 : 0) + (flags & AE_CHAIN_ENC ? (skip ? 0 : tmax_enc) : tmax);
}

// the token fed at chain step q of row b, 0 for AE2's image row (AutoEncoder_text_nostart.lua:249-262, :302-319; AutoEncoder.lua
// :258-291, :318-348).  enc: the stream the encoder reads (= dec but on the weak-paired archs); direct (decoding): the decoder's
// token from s = 1 on is direct[b], the last pick
NVQA_HD int chain_token(const AeChain &ch, const int32_t *enc, const int32_t *dec, const int32_t *direct, int q, int b)
{
    const int lead = ch.flags & AE_CHAIN_AE2 ? 2 : 0;
    int v;
    if (q < ch.te) {
        if (q < lead) return q == 0 ? 0 : ch.V + 1;
        v = enc[(size_t)b * ch.D + q - lead];
    } else {
        const int s = q - ch.te;
        if (s == 0) return ch.V + 1;
        v = direct ? direct[b] : dec[(size_t)b * ch.D + s - 1];
    }
    return v == 0 ? 1 : v;
}

// LanguageModelCriterion (AutoEncoder_text_nostart.lua:416-450), decoder step s = 0 .. D of one token row: the 0-based class --
// the token, END (= V) at the first null (position D counts as one) -- or -1 behind it
NVQA_HD int criterion_target(const int32_t *row, int s, int D, int V)
{
    const int v = s < D ? row[s] : 0;
    if (v != 0) return v - 1;
    for (int k = 0; k < s; ++k)
        if (row[k] == 0) return -1;
    return V;
}
// the row's steps with a target: every token and the first null, which position D always is
NVQA_HD int criterion_count(const int32_t *row, int D)
{
    int n = 1;
    for (int t = 0; t < D; ++t) n += row[t] != 0;
    return n;
}
// 1 + the row's last non-null column (0: a null row); tmax of a batch = the maximum over its rows
NVQA_HD int row_last(const int32_t *row, int D)
{
    while (D > 0 && row[D - 1] == 0) --D;
    return D;
}

// ---- host only ----
struct TokenFault { int value; int64_t row; int col; };

// src [n x D] (NULL: nulls) -> dst [B x D] (NULL: validate only), rows from n on zero; *tmax = the batch's.  false: the first
// value outside 0..V, in row order, in *what.
inline bool stage_tokens(const int32_t *src, int64_t n, int64_t B, int D, int V, int32_t *dst, int *tmax, TokenFault *what)
{
    *tmax = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int32_t *row = src && b < n ? src + (size_t)b * D : nullptr;
        for (int t = 0; t < D; ++t) {
            const int v = row ? row[t] : 0;
            if (v < 0 || v > V) { *what = {v, b, t}; return false; }
            if (dst) dst[(size_t)b * D + t] = v;
        }
        if (row && row_last(row, D) > *tmax) *tmax = row_last(row, D);
    }
    return true;
}

// The lookup gradient's index: a counting sort of the chain rows r = q B + b by chain_token (AE2: from row B on, the image row
// has none).  lk_tok [nu]: the distinct tokens ascending; lk_tc [nu + 1]: a token's first chunk; lk_start [nch + 1]: a chunk's
// first slot of lk_pos, chunks of at most NVQA_AE_LK_CHUNK rows inside one token; lk_pos: the rows, ascending inside a token.
inline void chain_index(const AeChain &ch, const int32_t *enc, const int32_t *dec, int32_t *lk_tok, int32_t *lk_tc,
                        int32_t *lk_start, int32_t *lk_pos, int32_t *nu_out, int32_t *nch_out)
{
    const int r_lo = ch.flags & AE_CHAIN_AE2 ? ch.B : 0, NP = (ch.te + ch.nd) * ch.B - r_lo;
    std::vector<int> ofs(ch.V + 2, 0), at(ch.V + 2, 0), tokr(NP);
    for (int i = 0; i < NP; ++i) {
        tokr[i] = chain_token(ch, enc, dec, nullptr, (r_lo + i) / ch.B, (r_lo + i) % ch.B);
        ++ofs[tokr[i]];
    }
    int nu = 0, nch = 0, acc = 0;
    for (int v = 1; v <= ch.V + 1; ++v) {
        if (!ofs[v]) continue;
        lk_tok[nu] = v;
        lk_tc[nu] = nch;
        for (int k = 0; k < ofs[v]; k += NVQA_AE_LK_CHUNK) lk_start[nch++] = acc + k;
        at[v] = acc;
        acc += ofs[v];
        ++nu;
    }
    lk_tc[nu] = nch;
    lk_start[nch] = acc;
    for (int i = 0; i < NP; ++i) lk_pos[at[tokr[i]]++] = r_lo + i;
    *nu_out = nu;
    *nch_out = nch;
}

} // namespace nvqa
