// kmajor_check_common.h -- TEST INFRASTRUCTURE: what the checkers of the K-major bf16 MFMA kernels share (wgrad_bf16_check.hip,
// wgrad_split_check.hip, wgrad_split2_check.hip, dx0_split_check.hip): the error-check macro, the two operand pools, the
// device kernels that fill operands, sum slabs and compute the f64 reference and the split-K f32 fmaf chain of a K-major
// product, the error norms, and the hash that ends every per-case line (bits=<16 hex digits>: FNV-1a over the output words,
// so that two builds of a kernel can be compared without a tolerance).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 3; }    \
    } while (0)

// the operand pools: dG log-normal x 1e-3; the other operand 2 tanh x Bernoulli(0.5), like Dropout(h)
inline float kc_lognormal(std::mt19937 &rng, std::normal_distribution<float> &nd)
{
    const float a = nd(rng), b = nd(rng);
    return a * expf(b) * 1e-3f;
}
inline float kc_tanh_bernoulli(std::mt19937 &rng, std::normal_distribution<float> &nd)
{
    const float a = nd(rng);
    return (rng() & 1u) ? 2.f * tanhf(a) : 0.f;
}

// FNV-1a over 32-bit words
inline uint64_t kc_fnv1a(const void *data, size_t words, uint64_t h = 0xcbf29ce484222325ull)
{
    const uint32_t *w = static_cast<const uint32_t *>(data);
    for (size_t i = 0; i < words; ++i) {
        uint32_t v = w[i];
        for (int b = 0; b < 4; ++b) { h = (h ^ (v & 0xffu)) * 0x100000001b3ull; v >>= 8; }
    }
    return h;
}

// operand [K][ld] from a pool of values; rows >= nrows[k / B] of a step: zero when zero_inactive
__global__ void k_fill(float *dst, int K, int ld, int cols, const float *pool, unsigned pool_n, const int *nrows, int B, int zero_inactive)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)K * ld) return;
    const int k = (int)(i / ld), c = (int)(i % ld);
    const bool on = !nrows || k % B < nrows[k / B];
    float v = pool[(unsigned)(((size_t)k * 2053 + c) % pool_n)];
    if (c >= cols) v = __builtin_nanf(""); // the padding between rows is never read
    if (!on && zero_inactive) v = 0.f;
    dst[i] = v;
}

// the slabs in z order
__global__ void k_sum_slabs(const float *slabs, int ks, size_t n, float *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int z = 0; z < ks; ++z) s += slabs[(size_t)z * n + i];
    out[i] = s;
}

// the reference of a K-major product A^T B: f64 products of the unrounded operands, f64 accumulation
__global__ void k_ref_f64(const float *A, const float *B, int lda, int ldb, int M, int N, int K, double *out)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (n >= N || m >= M) return;
    double s = 0;
    for (int k = 0; k < K; ++k) s += (double)A[(size_t)k * lda + m] * (double)B[(size_t)k * ldb + n];
    out[(size_t)m * N + n] = s;
}

// its f32 form: an fmaf chain per K slice, one slab per slice
__global__ void k_f32_chain(const float *A, const float *B, int lda, int ldb, int M, int N, int K, int kslice, float *slabs)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y, z = blockIdx.z;
    if (n >= N || m >= M) return;
    const int kend = min(K, (z + 1) * kslice);
    float s = 0.f;
    for (int k = z * kslice; k < kend; ++k) s = fmaf(A[(size_t)k * lda + m], B[(size_t)k * ldb + n], s);
    slabs[(size_t)z * M * N + (size_t)m * N + n] = s;
}

// L2-relative and max-relative error of c against ref (1e30 where c holds a NaN)
inline void errors(const std::vector<float> &c, const std::vector<double> &ref, double *l2, double *mx)
{
    double d2 = 0, r2 = 0, dm = 0, rm = 0;
    for (size_t i = 0; i < ref.size(); ++i) {
        const double d = (double)c[i] - ref[i];
        if (!(d == d)) { *l2 = *mx = 1e30; return; }
        d2 += d * d; r2 += ref[i] * ref[i];
        dm = fmax(dm, fabs(d)); rm = fmax(rm, fabs(ref[i]));
    }
    *l2 = sqrt(d2 / r2); *mx = dm / rm;
}
