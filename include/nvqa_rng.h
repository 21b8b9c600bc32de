/*
 * nvqa_rng.h -- counter-based dropout masks shared by the CPU oracle and the
 * HIP kernels (same bits on both sides, so training parity can be checked
 * with dropout active).  Replaces nn.Dropout's MT19937 bernoulli stream
 * (002_train_baseline.lua:143,153; misc/LSTM.lua:37; misc/netdef.lua:10-11),
 * which cannot be reproduced outside Torch7.
 *
 * keep(seed, step, site, idx) = u >= p with u uniform in [0,1) from a
 * splitmix64-style mix; kept elements are scaled by 1/(1-p) (nn.Dropout v2).
 *
 * Sites and element indices (b = sample row in the caller's batch order,
 * t = 0-based column of the question buffer, independent of the length sort):
 *   NVQA_SITE_EMB  arch1 word embedding   idx = (b*T + t)*E + e
 *   NVQA_SITE_LSTM input of layer l >= 2  idx = (((l-2)*B + b)*Tsteps + t)*R + j
 *                  (arch2: Tsteps = T+2 and t is the encoder step)
 *   NVQA_SITE_Q    question vector        idx = b*(2RL) + j   (arch2: b*R + j, head dropout)
 *   NVQA_SITE_V    image feature          idx = b*I + j
 *   NVQA_SITE_Z    fused vector           idx = b*C + j
 * Text auto-encoder (NVQA_ARCH_AE1; D = seq_length, s = decoder step 0..D, k = 0 encoder / 1 decoder):
 *   NVQA_SITE_AE_ENC_LK   encoder lookup        idx = (b*D + t)*E + e
 *   NVQA_SITE_AE_DEC_LK   decoder lookup        idx = (b*(D+1) + s)*E + e
 *   NVQA_SITE_AE_TOP      decoder top h         idx = (b*(D+1) + s)*R + j
 *   NVQA_SITE_AE_LSTM     input of layer l >= 1 idx = (((k*L + l)*B + b)*(D+1) + t)*R + j
 * Image-first-token auto-encoder (NVQA_ARCH_AE2): the encoder runs up to D+2 steps (image, START, tokens), so the
 * step stride is D+2; the lookup is a plain LookupTable and draws no mask (no ENC_LK / DEC_LK):
 *   NVQA_SITE_AE_TOP      decoder top h         idx = (b*(D+2) + s)*R + j
 *   NVQA_SITE_AE_LSTM     input of layer l >= 1 idx = (((k*L + l)*B + b)*(D+2) + t)*R + j   (encoder t = 0..D+1)
 * The weak-paired auto-encoder (NVQA_ARCH_AE2_WP) draws the NVQA_ARCH_AE2 masks with the same indices.
 * Decoding (nvqa_ae_sample / nvqa_ae_sample_rows, mode 1; seed and step are nvqa_sample_opts'): no mask but the uniform of the
 * multinomial draw, u = (hash32 >> 8) * 2^-24, one per emitted token (b = row in the caller's order, s = 0..D-1):
 *   NVQA_SITE_AE_SAMPLE   sample position        idx = b*D + s
 * The VGG-16 body in training mode (nvqa_vgg16_fc7_raw and the weak-paired *_images steps with a body dropout; F = the fc width,
 * b = image row in the caller's order; seed and step are the body dropout's own):
 *   NVQA_SITE_VGG_FC6     drop6 (module 35)      idx = b*F + j
 *   NVQA_SITE_VGG_FC7     drop7 (module 38)      idx = b*F + j
 */
#ifndef NVQA_RNG_H
#define NVQA_RNG_H

#include <stdint.h>

#if defined(__HIPCC__)
#define NVQA_HD __host__ __device__ __forceinline__
#else
#define NVQA_HD static inline
#endif

#define NVQA_SITE_EMB 0u
#define NVQA_SITE_LSTM 1u
#define NVQA_SITE_Q 2u
#define NVQA_SITE_V 3u
#define NVQA_SITE_Z 4u
#define NVQA_SITE_AE_ENC_LK 5u
#define NVQA_SITE_AE_DEC_LK 6u
#define NVQA_SITE_AE_TOP 7u
#define NVQA_SITE_AE_LSTM 8u
#define NVQA_SITE_AE_SAMPLE 9u
#define NVQA_SITE_VGG_FC6 10u
#define NVQA_SITE_VGG_FC7 11u

NVQA_HD uint32_t nvqa_hash32(uint64_t seed, uint64_t step, uint32_t site, uint64_t idx)
{
    uint64_t x = seed ^ (0x9E3779B97F4A7C15ULL * (step + 1ULL)) ^ ((uint64_t)site << 56);
    x += idx * 0xD1342543DE82EF95ULL;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

/* multiplier applied to the element: 0 or 1/(1-p) */
NVQA_HD float nvqa_dropout_scale(uint64_t seed, uint64_t step, uint32_t site, uint64_t idx, float p,
                                 float inv_keep)
{
    const float u = (float)(nvqa_hash32(seed, step, site, idx) >> 8) * (1.0f / 16777216.0f);
    return u >= p ? inv_keep : 0.0f;
}

#endif /* NVQA_RNG_H */
