// ae_decode.h -- the selection kernels of nvqa_ae_sample / nvqa_ae_sample_rows (NVQA_ARCH_AE1 / NVQA_ARCH_AE2; DESIGN.md
// section 9.9): what sample(sents, opt) of misc/AutoEncoder_text_nostart.lua:134-210 does behind a decoder step's logits --
// argmax or a multinomial draw at a temperature, and the log-probability of the emitted token -- and the library's own beam
// search (the reference names sample_beam at :138 and does not ship it).
//
// One workgroup of 256 threads per decoder row.  The row of V + 1 <= 16384 f32 logits is read once and kept in registers:
// thread t owns the 4 NV4 columns from 4 NV4 t on.  The ownership is contiguous on purpose: the multinomial pick is defined
// on the CDF in column order, so a prefix over the threads' sums followed by a walk through the owner's registers is that
// CDF.  Max and sum-exp are found together (an online pair per thread, 64-lane butterflies, one LDS combine that every
// thread repeats in the same order).  No atomics anywhere: every result is a fixed function of the row's bits.
//
// With z the row, l = z - logsumexp(z):
//   mode 0  pick = first maximum of z (k_ae_argmax's rule), log-prob l[pick]
//   mode 1  w_c = exp((z_c - max z) / T), u from nvqa_hash32(seed, step, NVQA_SITE_AE_SAMPLE, b D + s); pick = the smallest c
//           with w_c > 0 and CDF(c) > u CDF(V), CDF in this kernel's order (the owner's exclusive prefix, then its columns one
//           by one); none (rounding) -> the last c with w_c > 0.  The log-prob is the untempered l[pick] (logprobs:gather, :195)
//   mode 2  the row's K best (S + l_c, c), S the hypothesis' score, ties to the smaller c; k_ae_beam_merge ranks a sentence's
//           candidates, k_ae_beam_gather re-orders the recurrent state, k_ae_beam_out walks the back-pointers
#ifndef NVQA_AE_DECODE_H
#define NVQA_AE_DECODE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nvqa_rng.h"

namespace nvqa {

constexpr int NVQA_AE_BEAM_MAX = 8;    // beam_size <= 8: a sentence's K x K candidates fit one wave
constexpr int NVQA_AE_SEL_NT = 256;    // threads per row
constexpr int NVQA_AE_SEL_MAXV4 = 16;  // float4s a thread holds at most: rows of up to 256 x 64 = 16384 columns

__device__ __forceinline__ void dec_lse_combine(float &m, float &s, float m2, float s2)
{
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) { m = m2; s = s2; return; }
    if (m2 > m) { s = s * expf(m - m2) + s2; m = m2; }
    else s += s2 * expf(m2 - m);
}

// the thread's columns [c0, c0 + 4 NV4) of the row; columns from Vp1 on read as -inf
template <int NV4>
__device__ __forceinline__ void dec_row_load(const float *x, int ldl, int Vp1, int c0, float (&v)[4 * NV4])
{
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
        const int c = c0 + 4 * i;
        const float4 q = c < ldl ? x4[c >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * i] = c < Vp1 ? q.x : -INFINITY;
        v[4 * i + 1] = c + 1 < Vp1 ? q.y : -INFINITY;
        v[4 * i + 2] = c + 2 < Vp1 ? q.z : -INFINITY;
        v[4 * i + 3] = c + 3 < Vp1 ? q.w : -INFINITY;
    }
}

// max, sum exp(z - max) and the first maximum's column of the whole row, the same bits in every thread
template <int N>
__device__ __forceinline__ void dec_row_stats(const float (&v)[N], int c0, float &M, float &S, int &A, float *sm, float *ss, int *sa)
{
    float m = -INFINITY, s = 0.f;
    int am = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (v[k] > m) { m = v[k]; am = c0 + k; }
    if (m != -INFINITY) {
#pragma unroll
        for (int k = 0; k < N; ++k) s += expf(v[k] - m); // (exp(-inf) = 0 behind the row's end)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const int a2 = __shfl_xor(am, o, 64);
        if (m2 > m || (m2 == m && a2 < am)) am = a2;
        dec_lse_combine(m, s, m2, s2);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w] = m; ss[w] = s; sa[w] = am; }
    __syncthreads();
    M = sm[0]; S = ss[0]; A = sa[0];
    for (int k = 1; k < NVQA_AE_SEL_NT / 64; ++k) {
        if (sm[k] > M || (sm[k] == M && sa[k] < A)) A = sa[k];
        dec_lse_combine(M, S, sm[k], ss[k]);
    }
}

// modes 0 and 1 on the logits of decoder step s, rows [0, gridDim.x): the pick (1-based) goes to cur (the next step's input)
// and to samples[b][s], its log-probability to slp[b][s]
template <int NV4>
__global__ __launch_bounds__(NVQA_AE_SEL_NT) void k_ae_select(const float *logits, int ldl, int Vp1, int D, int s, int mode, float temperature,
                                                              uint64_t seed, uint64_t step, int32_t *cur, int32_t *samples, float *slp)
{
    constexpr int N = 4 * NV4, NW = NVQA_AE_SEL_NT / 64;
    __shared__ float sm[NW], ss[NW], wt[NW];
    __shared__ int sa[NW], sh[NW];
    const int b = blockIdx.x, c0 = threadIdx.x * N, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float v[N];
    dec_row_load<NV4>(logits + (size_t)b * ldl, ldl, Vp1, c0, v);
    float M, S;
    int A;
    dec_row_stats<N>(v, c0, M, S, A, sm, ss, sa);
    const float lse = M + logf(S);
    const size_t o = (size_t)b * D + s;
    if (mode == 0) {
        if (threadIdx.x == 0) { cur[b] = A + 1; samples[o] = A + 1; slp[o] = M - lse; }
        return;
    }
    // the thread's weights replace its logits; zv keeps what the outputs need: the logits of its first hit and of its last w > 0
    float tsum = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) tsum += c0 + k < Vp1 ? expf((v[k] - M) / temperature) : 0.f;
    float incl = tsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const float prev = __shfl_up(incl, 1, 64);
    if (lane == 63) wt[w] = incl;
    __syncthreads();
    float base = 0.f, total = 0.f;
    for (int k = 0; k < NW; ++k) {
        if (k == w) base = total;
        total += wt[k];
    }
    const float u = (float)(nvqa_hash32(seed, step, NVQA_SITE_AE_SAMPLE, (uint64_t)b * D + s) >> 8) * (1.0f / 16777216.0f);
    const float target = u * total;
    float run = base + (lane ? prev : 0.f), zhit = 0.f, zlast = 0.f;
    int hit = 0x7fffffff, last = -1;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float wk = c0 + k < Vp1 ? expf((v[k] - M) / temperature) : 0.f;
        run += wk;
        if (wk > 0.f) {
            last = c0 + k; zlast = v[k];
            if (run > target && hit == 0x7fffffff) { hit = c0 + k; zhit = v[k]; }
        }
    }
    int bh = hit, bl = last;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        bh = min(bh, __shfl_xor(bh, d, 64));
        bl = max(bl, __shfl_xor(bl, d, 64));
    }
    if (lane == 0) { sa[w] = bh; sh[w] = bl; } // (sa: every thread has read the maxima's columns before the barrier above)
    __syncthreads();
    for (int k = 0; k < NW; ++k) { bh = min(bh, sa[k]); bl = max(bl, sh[k]); }
    if (bh != 0x7fffffff) {
        if (hit == bh) { cur[b] = bh + 1; samples[o] = bh + 1; slp[o] = zhit - lse; }
    } else if (last == bl && bl >= 0) {
        cur[b] = bl + 1; samples[o] = bl + 1; slp[o] = zlast - lse;
    }
}

// mode 2, rows [0, gridDim.x) = the live hypotheses' decoder rows (row r = sentence r / K, hypothesis r % K): the row's K best
// (S_r + l_c, c), best first, ties to the smaller c, into cand_*[r][0 .. K).  At position 0 only hypothesis 0 of a sentence is
// expanded (S = 0); a finished hypothesis offers itself in k_ae_beam_merge and is skipped here.
template <int NV4>
__global__ __launch_bounds__(NVQA_AE_SEL_NT) void k_ae_beam_rows(const float *logits, int ldl, int Vp1, int s, int K, const float *score,
                                                                 const int32_t *fin, float *cand_sc, float *cand_lp, int32_t *cand_c)
{
    constexpr int N = 4 * NV4, NW = NVQA_AE_SEL_NT / 64;
    __shared__ float sm[NW], ss[NW], sz[NW];
    __shared__ int sa[NW];
    const int r = blockIdx.x, c0 = threadIdx.x * N, w = threadIdx.x >> 6;
    if (s == 0 ? r % K != 0 : fin[r] != 0) return;
    float v[N];
    dec_row_load<NV4>(logits + (size_t)r * ldl, ldl, Vp1, c0, v);
    float M, S;
    int A;
    dec_row_stats<N>(v, c0, M, S, A, sm, ss, sa);
    const float lse = M + logf(S), S_r = s == 0 ? 0.f : score[r];
    for (int j = 0; j < K; ++j) {
        float bs = -INFINITY, bz = 0.f;
        int bc = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float sc = S_r + (v[k] - lse);
            if (sc > bs) { bs = sc; bc = c0 + k; bz = v[k]; }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float s2 = __shfl_xor(bs, d, 64), z2 = __shfl_xor(bz, d, 64);
            const int c2 = __shfl_xor(bc, d, 64);
            if (s2 > bs || (s2 == bs && c2 < bc)) { bs = s2; bc = c2; bz = z2; }
        }
        __syncthreads(); // the last round's (and dec_row_stats') reads of the arrays are done
        if ((threadIdx.x & 63) == 0) { sm[w] = bs; sa[w] = bc; sz[w] = bz; }
        __syncthreads();
        bs = sm[0]; bc = sa[0]; bz = sz[0];
        for (int k = 1; k < NW; ++k)
            if (sm[k] > bs || (sm[k] == bs && sa[k] < bc)) { bs = sm[k]; bc = sa[k]; bz = sz[k]; }
        if (threadIdx.x == 0) {
            const size_t o = (size_t)r * NVQA_AE_BEAM_MAX + j;
            cand_sc[o] = bs; cand_c[o] = bc; cand_lp[o] = bz - lse;
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (c0 + k == bc) v[k] = -INFINITY;
    }
}

// mode 2, one wave per sentence i: ranks the live hypotheses' K candidates each and the finished hypotheses' self-offers (score
// unchanged, ranked as (k, END)) by score, ties to the smaller k (V + 1) + c, and keeps the K best, best first.  Survivor p gets
// its back-pointer (the parent's decoder row), its token (0 behind END) and log-prob at position s, its score, its finished flag
// and the token its row is fed next.  Every read of score / fin precedes the barrier, every write follows it.
__global__ __launch_bounds__(64) void k_ae_beam_merge(int K, int s, int B, int Vp1, const float *cand_sc, const float *cand_lp,
                                                      const int32_t *cand_c, float *score, int32_t *fin, int32_t *cur, int32_t *bp,
                                                      int32_t *tk, float *lp)
{
    __shared__ float ssc[64];
    __shared__ int skey[64];
    const int i = blockIdx.x, t = threadIdx.x, k = t / K, j = t % K, r = i * K + (k < K ? k : 0);
    bool valid = false, self = false;
    float sc = -INFINITY, l = 0.f;
    int c = 0;
    if (t < K * K) {
        const bool done = s > 0 && fin[r] != 0;
        if (s == 0 ? k == 0 : !done) {
            const size_t o = (size_t)r * NVQA_AE_BEAM_MAX + j;
            valid = true; sc = cand_sc[o]; c = cand_c[o]; l = cand_lp[o];
        } else if (done && j == 0) {
            valid = self = true; sc = score[r]; c = Vp1 - 1;
        }
    }
    const int key = valid ? k * Vp1 + c : 0x7fffffff;
    ssc[t] = sc; skey[t] = key;
    __syncthreads();
    if (!valid) return;
    int rank = 0;
    for (int q = 0; q < K * K; ++q)
        if (skey[q] != 0x7fffffff && (ssc[q] > sc || (ssc[q] == sc && skey[q] < key))) ++rank;
    if (rank >= K) return;
    const int p = i * K + rank;
    const size_t o = (size_t)s * B + p;
    bp[o] = r;
    tk[o] = self ? 0 : c + 1;
    lp[o] = self ? 0.f : l;
    score[p] = sc;
    fin[p] = self || c == Vp1 - 1;
    cur[p] = c + 1;
}

// rows [0, rows) of dst = rows bp[r] of src (bp NULL: r / K, the encoder's final state of sentence r / K to its K decoder rows),
// h and c of one layer, 16 bytes a thread.  src and dst are different buffers: the step writes a state slot, the gather reads it
// into the buffer the next step reads.
__global__ void k_ae_beam_gather(const float *src_h, const float *src_c, float *dst_h, float *dst_c, const int32_t *bp, int K, int rows,
                                 int R4)
{
    const size_t n = (size_t)rows * R4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / R4), j = (int)(i % R4);
        const size_t src = (size_t)(bp ? bp[r] : r / K) * R4 + j;
        reinterpret_cast<float4 *>(dst_h)[i] = reinterpret_cast<const float4 *>(src_h)[src];
        reinterpret_cast<float4 *>(dst_c)[i] = reinterpret_cast<const float4 *>(src_c)[src];
    }
}

// mode 2: hypothesis 0 of every sentence, walked back through the back-pointers; zeros behind END come from the self-offers
__global__ void k_ae_beam_out(int n, int K, int D, int B, const int32_t *bp, const int32_t *tk, const float *lp, int32_t *samples,
                              float *slp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = i * K;
    for (int s = D - 1; s >= 0; --s) {
        const size_t o = (size_t)s * B + r;
        samples[(size_t)i * D + s] = tk[o];
        slp[(size_t)i * D + s] = lp[o];
        r = bp[o];
    }
}

} // namespace nvqa

#endif /* NVQA_AE_DECODE_H */
