// vgg_bwd.h -- the kernels of the VGG-16 body's backward pass and update (vgg.hip; f32 body only).
//
// Replaces protos.cnn:backward(data.imgs, dfeats) and the cnn branch of the update of
// 004_train_arch{1,2}_weakpaired_autoencoder_vgg.lua (arch2 :307-310, :457-466; arch1 :329, :477-484): the cudnn
// SpatialConvolution / ReLU / SpatialMaxPooling / Linear / Dropout backward chain and misc/optim_updates.lua's lrs forms.
//
// The dense products run on the f32 MFMA template of gemm_f32.h:
//   dX of a convolution = the forward implicit GEMM on dZ with the tap-flipped, channel-swapped weight image W' (EpiGradMask);
//   dW of a convolution = A_MC x B_NCTAP: dW[co][tap][ci] = sum_pixels dZ[pixel][co] X[pixel + tap][ci], K = n H W, split over K
//                         into slabs that k_vgg_slab_sum adds in slab order (no atomics: a backward is bit-reproducible);
//   fc6 / fc7: dA = dZ W (A_KC x B_NC), dW = dZ^T A (A_MC x B_NC, K = n: memory-bound).
// The ReLU and Dropout masks are read off the stored post-ReLU, post-dropout outputs: a kept, positive unit is exactly a
// positive stored value, so no mask is kept or redrawn.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nvqa.h"
#include "gemm_f32.h"

namespace nvqa {

// dW of a convolution: M = C_out, N = 9 C_in_pad, K = pixels, both operands contiguous along the output dimensions; the 32x32x2
// MFMA form the other long-K weight gradients of the library use.  A staged float4 of the X operand keeps its tap over the whole
// K loop (gemm_f32.h B_NCTAP), so one loader serves C_in_pad = 4 (conv1_1), the narrow networks and the full-width layers alike.
typedef Cfg<32, 128, 128, 32, 2, 2, 1, 1> CfgVggDw;   // C_out > 64
typedef Cfg<32, 64, 128, 32, 1, 4, 1, 1> CfgVggDw64;  // C_out <= 64

// dX epilogue: store, or store x [y_below > 0] (y = the stored output of the layer below, same NHWC shape) when no pool lies between
struct EpiGradMask {
    float *C;
    int ldc;
    const float *y;
    __device__ __forceinline__ void operator()(int, int m, int n, float v) const
    {
        const size_t o = (size_t)m * ldc + n;
        C[o] = (!y || y[o] > 0.0f) ? v : 0.0f;
    }
};

// nn.L2Normalize:updateGradInput (misc/L2Normalize.lua:22-40) row by row: dx = (r^2 I - f f^T) / r^3 dy = dy / r - f (f . dy) / r^3
// with r = |f| of the stored features.  One wave per row.  A row of norm zero: the forward (k_l2norm_rows) divides by zero as the
// module does and yields NaN, and so does this.
__global__ void k_vgg_l2norm_bwd(const float *dy, const float *f, int n, int F, float *dx)
{
    const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (row >= n) return;
    const float *fr = f + (size_t)row * F, *dr = dy + (size_t)row * F;
    float ss = 0.f, dot = 0.f;
    for (int i = lane; i < F; i += 64) {
        ss += fr[i] * fr[i];
        dot += fr[i] * dr[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o, 64);
        dot += __shfl_xor(dot, o, 64);
    }
    const float r = sqrtf(ss), r3 = r * r * r;
    for (int i = lane; i < F; i += 64) dx[(size_t)row * F + i] = dr[i] / r - fr[i] * dot / r3;
}

// ReLU + Dropout backward of an fc layer from its stored output: dZ = dY (y > 0 ? s : 0), s = 1 / keep of a live dropout, else 1
__global__ void k_vgg_fc_dz(const float *dY, const float *y, float s, size_t count, float *dZ)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dZ[i] = y[i] > 0.0f ? dY[i] * s : 0.0f;
}

// sum of S split-K slabs in slab order; with y the fc mask of k_vgg_fc_dz applied to the sum
__global__ void k_vgg_slab_sum(const float *slabs, int S, size_t count, const float *y, float s, float *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float a = 0.f;
    for (int z = 0; z < S; ++z) a += slabs[(size_t)z * count + i];
    out[i] = !y ? a : (y[i] > 0.0f ? a * s : 0.0f);
}

// SpatialMaxPooling(2, 2, 2, 2) backward fused with the ReLU below it: the gradient of a pooled value goes to the FIRST maximum of
// its window in row-major order (Torch's rule) and is multiplied by [a > 0]; the three other positions get zero.  a: the stored
// post-ReLU convolution output [n][H][W][4 C4], dP [n][H/2][W/2][4 C4]; every position of dZ is written.  Pad channels hold
// a = 0 and so get zero.
__global__ void k_vgg_pool_relu_bwd(const float4 *a, const float4 *dP, int n, int H, int W, int C4, float4 *dZ)
{
    const int Ho = H / 2, Wo = W / 2;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * Ho * Wo * C4) return;
    const int c = i % C4;
    size_t p = i / C4;
    const int x = p % Wo; p /= Wo;
    const int y = p % Ho; const size_t img = p / Ho;
    const size_t o0 = ((img * H + 2 * y) * W + 2 * x) * C4 + c;
    const size_t o[4] = {o0, o0 + C4, o0 + (size_t)W * C4, o0 + (size_t)W * C4 + C4};
    const float4 v[4] = {a[o[0]], a[o[1]], a[o[2]], a[o[3]]};
    const float4 g = dP[i];
    float4 r[4];
    auto one = [](float v0, float v1, float v2, float v3, float gg, float &r0, float &r1, float &r2, float &r3) {
        const float mx = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        const int k = v0 == mx ? 0 : (v1 == mx ? 1 : (v2 == mx ? 2 : 3));
        const float gv = mx > 0.0f ? gg : 0.0f;
        r0 = k == 0 ? gv : 0.0f; r1 = k == 1 ? gv : 0.0f; r2 = k == 2 ? gv : 0.0f; r3 = k == 3 ? gv : 0.0f;
    };
    one(v[0].x, v[1].x, v[2].x, v[3].x, g.x, r[0].x, r[1].x, r[2].x, r[3].x);
    one(v[0].y, v[1].y, v[2].y, v[3].y, g.y, r[0].y, r[1].y, r[2].y, r[3].y);
    one(v[0].z, v[1].z, v[2].z, v[3].z, g.z, r[0].z, r[1].z, r[2].z, r[3].z);
    one(v[0].w, v[1].w, v[2].w, v[3].w, g.w, r[0].w, r[1].w, r[2].w, r[3].w);
#pragma unroll
    for (int k = 0; k < 4; ++k) dZ[o[k]] = r[k];
}

// W [C_out][9][C_in_pad] -> W' [C_in][9][C_out_pad]: taps flipped (tap' = 8 - tap), channels swapped, pad channels zero: the
// weight image with which the forward implicit GEMM on dZ gives dX.  Rebuilt after every change of W.
__global__ void k_vgg_repack_wt(const float *W, int cout, int cin, int cinp, int coutp, float *Wt)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)cin * 9 * coutp) return;
    const int co = i % coutp, tap = (i / coutp) % 9, ci = i / ((size_t)9 * coutp);
    Wt[i] = co < cout ? W[((size_t)co * 9 + (8 - tap)) * cinp + ci] : 0.0f;
}

// column sums of X [M][ld] (bias gradients), two stages, fixed order: kernels.h's k_colsum_part / k_colsum_final restated for
// this translation unit (kernels.h belongs to the VQA step's context).  Stage 1: grid (N / 64, S), a block of 4 waves sums its
// row stripe for 64 columns (wave w takes rows w, w + 4, ..., four chains each) -> part[s][n]; stage 2 adds the S <= 128 partials.
__global__ __launch_bounds__(256) void k_vgg_colsum_part(const float *X, int M, int N, int ld, int rps, float *part)
{
    __shared__ float sm[4][64];
    const int n = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
    const int mbeg = blockIdx.y * rps, mend = min(M, mbeg + rps);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (n < N) {
        int m = mbeg + w;
        for (; m + 12 < mend; m += 16) {
            s0 += X[(size_t)m * ld + n];
            s1 += X[(size_t)(m + 4) * ld + n];
            s2 += X[(size_t)(m + 8) * ld + n];
            s3 += X[(size_t)(m + 12) * ld + n];
        }
        for (; m < mend; m += 4) s0 += X[(size_t)m * ld + n];
    }
    sm[w][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (w == 0 && n < N) part[(size_t)blockIdx.y * N + n] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}
__global__ void k_vgg_colsum_final(const float *part, int S, int N, float *out)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += part[(size_t)i * N + n];
    out[n] = s;
}

// The lrs forms of misc/optim_updates.lua (sgd :4-10, sgdm :12-24, adam :78-111) on one repacked array, every step multiplied by
// `scale` (cnnFinalLearningScales): g += wd scale x, clamp, the rule -- the script's order.  Element i is a true weight when
// i % period < real (the channel padding of the repacked layouts); pad lanes are left alone: their weight, gradient and state
// are zero.  part[2 blk] = sum x^2, part[2 blk + 1] = count(|lr g| >= 0.01 |x|), of x before the update and g after wd and clamp.
struct VggRule {
    float lr, b1, b2, eps, step; // step: Adam's bias-corrected rate (formed on the host)
};
template <int RULE>
__global__ __launch_bounds__(256) void k_vgg_optim(float *x, float *m, float *v, const float *g, size_t n, int period, int real, VggRule r,
                                                   float wd, float clamp, float scale, double *part)
{
    __shared__ double sh[2][256];
    double sq = 0, cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if ((int)(i % period) >= real) continue;
        float xi = x[i], gi = g[i];
        if (wd != 0.f) gi += wd * (xi * scale);
        if (clamp > 0.f) gi = fminf(fmaxf(gi, -clamp), clamp);
        sq += (double)xi * (double)xi;
        cnt += fabsf(gi * r.lr) >= fabsf(xi) * 0.01f ? 1.0 : 0.0;
        if constexpr (RULE == NVQA_OPT_SGD) {
            xi += -r.lr * (gi * scale);
        } else if constexpr (RULE == NVQA_OPT_SGDM) {
            const float mi = r.b1 * m[i] + r.lr * (gi * scale);
            m[i] = mi;
            xi -= mi;
        } else {
            const float mi = r.b1 * m[i] + (1.f - r.b1) * gi, vi = r.b2 * v[i] + (1.f - r.b2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            xi -= r.step * ((mi / (sqrtf(vi) + r.eps)) * scale);
        }
        x[i] = xi;
    }
    sh[0][threadIdx.x] = sq;
    sh[1][threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = sh[0][0]; part[2 * blockIdx.x + 1] = sh[1][0]; }
}

} // namespace nvqa
