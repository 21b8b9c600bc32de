// ae_bridge.h -- the state bridge of the arch1 weak-paired auto-encoder (NVQA_ARCH_AE1_WP, ae.hip): between the encoder's
// final state j = [c_T | h_T] and the decoder's initial state sits netdef.AxB(2R, I, 2R, 0.5) -> Dropout(0.5) and two
// CAddTables (001_train_autoencoder/misc/AutoEncoder_vqa_arch.lua:35-40, forward :337-350, backward :428-443):
//   qd = D_Q j, vd = D_V f^, qc = tanh(qd W_q^T + b_q), ic = tanh(vd W_v^T + b_v), m = D_Z (qc * ic),
//   c0_dec = c_T + m[:, :R], h0_dec = h_T + m[:, R:].
// The two projections have M = B rows (16 / 10 in the scripts) against K = 2R and K = I = 4096: as 64-wide tiles they would walk
// K serially on 16 workgroups.  They run here as ONE split-K launch over both problems (k_ae1wp_bridge_gemv): a wave owns 16
// output columns and one K slice, streams its 16 weight rows from memory straight into the f32 MFMA's operand registers (no
// LDS round trip: every weight element is used once) and writes a [B x 16] partial into its slab.  The slabs are summed in a
// fixed order at the launch boundary by the finisher k_ae1wp_bridge_fwd, which also adds the biases, applies tanh, the product
// and D_Z, adds the encoder's state and writes the decoder's initial state slot.  No atomics, no fences: bit-reproducible.
// Batches of more than 16 rows take the LDS-tiled wide form (ae.hip) into the same slabs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epilogues.h"
#include "gemm_f32.h"

namespace nvqa {

// K slice of both products and the slabs it gives.  skinny: k_ae1wp_bridge_gemv (B <= 16), else 128 x 128 tiles.  The slice
// is halved from 1024 until the launch has a wave per SIMD (skinny) / a workgroup per CU (wide), or 64 is reached.
struct BridgePlan {
    int skinny = 0, ks = 0, zq = 0, zv = 0, workgroups = 0;
};
inline BridgePlan ae1wp_bridge_plan(int B, int N, int Kq, int Kv, int num_cus)
{
    BridgePlan p;
    p.skinny = B <= 16;
    const int tiles = p.skinny ? (N + 15) / 16 : ((B + 127) / 128) * ((N + 127) / 128);
    const int want = p.skinny ? 4 * num_cus : num_cus;
    p.ks = 1024;
    while (p.ks > 64 && tiles * ((Kq + p.ks - 1) / p.ks + (Kv + p.ks - 1) / p.ks) < want) p.ks /= 2;
    p.zq = (Kq + p.ks - 1) / p.ks;
    p.zv = (Kv + p.ks - 1) / p.ks;
    p.workgroups = p.skinny ? (tiles * (p.zq + p.zv) + 3) / 4 : tiles * (p.zq + p.zv);
    return p;
}

// D_Q on the joined state, D_V on the features (netdef.AxB's two Dropouts).  cT != NULL: j = [cT | hT] is formed here (the
// encoder ran); NULL: j holds the caller's state already (encoder_skip_flag = 1).
__global__ void k_ae1wp_bridge_prep(const float *cT, const float *hT, float *j, const float *fhat, int B, int R, int I, Drop dr,
                                    float *qd, float *vd)
{
    const size_t nq = (size_t)B * 2 * R, nv = (size_t)B * I;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq + nv; i += (size_t)gridDim.x * blockDim.x) {
        if (i < nq) {
            const int b = (int)(i / (2 * R)), k = (int)(i % (2 * R));
            float v;
            if (cT) {
                v = k < R ? cT[(size_t)b * R + k] : hT[(size_t)b * R + k - R];
                j[i] = v;
            } else v = j[i];
            qd[i] = dr.scale(NVQA_SITE_Q, i) * v;
        } else {
            const size_t o = i - nq;
            vd[o] = dr.scale(NVQA_SITE_V, o) * fhat[o];
        }
    }
}

// Both projections, split-K, for B <= 16 rows.  Problem p: slab[p][z][b][n] = sum over the K slice z of x[p][b][k] w[p][n][k].
// A wave = (problem, K slice, 16 columns n0 ..); lane (li, lh) = (lane % 16, lane / 16) loads the float4 at k = k0 + 16 u + 4 lh
// of weight row n0 + li and of x row li (zeros beyond B) and feeds component w of both to MFMA w of q step u: in one
// v_mfma_f32_16x16x4_f32 lane group lh supplies k index lh for both operands, so any k order works as long as it is the same
// for both.  Result layout (gemm_f32.h): register r of lane (li, lh) = C[row 4 lh + r][column li].
struct BridgeGemvArgs {
    const float *x[2]; // qd [B x K0], vd [B x K1]
    const float *w[2]; // W_q [N x K0], W_v [N x K1]
    float *slab[2];    // [Z][B][N]
    int K[2], Z[2];
    int B, N, ks;      // ks % 64 == 0; K % 4 == 0; 16-byte aligned rows
};
__global__ __launch_bounds__(256) void k_ae1wp_bridge_gemv(BridgeGemvArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = (a.N + 15) / 16;
    int t = blockIdx.x * 4 + wave, p = 0;
    if (t >= nt * a.Z[0]) { p = 1; t -= nt * a.Z[0]; }
    if (t >= nt * a.Z[p]) return; // (wave-uniform; no barrier in this kernel)
    const int z = t / nt, n0 = (t % nt) * 16;
    const int K = a.K[p], kbeg = z * a.ks, kend = min(K, kbeg + a.ks);
    const int li = lane & 15, lh = lane >> 4;
    const bool xok = li < a.B, wok = n0 + li < a.N;
    const float *xr = a.x[p] + (size_t)(xok ? li : 0) * K;
    const float *wr = a.w[p] + (size_t)(wok ? n0 + li : 0) * K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8; // q steps (16 k each) whose loads are in flight together
    for (int k0 = kbeg; k0 < kend; k0 += 16 * U) {
        float4 xv[U], wv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + 16 * u + 4 * lh; // k % 4 == 0 and K % 4 == 0: k < kend covers the whole float4
            const bool in = k < kend;
            wv[u] = in && wok ? *reinterpret_cast<const float4 *>(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            xv[u] = in && xok ? *reinterpret_cast<const float4 *>(xr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc = mfma<16>(xv[u].x, wv[u].x, acc);
            acc = mfma<16>(xv[u].y, wv[u].y, acc);
            acc = mfma<16>(xv[u].z, wv[u].z, acc);
            acc = mfma<16>(xv[u].w, wv[u].w, acc);
        }
    }
    if (!wok) return;
    float *out = a.slab[p] + (size_t)z * a.B * a.N + n0 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = 4 * lh + r;
        if (b < a.B) out[(size_t)b * a.N] = acc[r];
    }
}

// The finisher: slab sums in slice order + bias, tanh, product, D_Z, + the encoder's state, straight into the decoder's initial
// state slot (c0, h0: [B x R] each); qc and ic are kept for the backward pass.
__global__ void k_ae1wp_bridge_fwd(const float *sq, int Zq, const float *sv, int Zv, int B, int R, const float *bq, const float *bv,
                                   const float *j, Drop dr, float *qc, float *ic, float *c0, float *h0)
{
    const size_t n = (size_t)B * 2 * R, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / (2 * R)), k = (int)(i % (2 * R));
    float q = 0.f, v = 0.f;
    for (int z = 0; z < Zq; ++z) q += sq[(size_t)z * n + i];
    for (int z = 0; z < Zv; ++z) v += sv[(size_t)z * n + i];
    q = tanhf_(q + bq[k]);
    v = tanhf_(v + bv[k]);
    qc[i] = q;
    ic[i] = v;
    const float s = j[i] + dr.scale(NVQA_SITE_Z, i) * (q * v);
    if (k < R) c0[(size_t)b * R + k] = s;
    else h0[(size_t)b * R + k - R] = s;
}

// Backward of the CAddTables' second inputs, Dropout, CMulTable and the two Tanh in one pass: dc = the cell gradient BPTT
// carried out of decoder step 0, dh0 = that step's dG W_h2h product.
__global__ void k_ae1wp_bridge_bwd(const float *dc, const float *dh0, const float *qc, const float *ic, int B, int R, Drop dr,
                                   float *dqp, float *dvp)
{
    const size_t n = (size_t)B * 2 * R, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / (2 * R)), k = (int)(i % (2 * R));
    const float g = k < R ? dc[(size_t)b * R + k] : dh0[(size_t)b * R + k - R];
    const float dz = dr.scale(NVQA_SITE_Z, i) * g, q = qc[i], v = ic[i];
    dqp[i] = dz * v * (1.0f - q * q);
    dvp[i] = dz * q * (1.0f - v * v);
}

// dj = D_Q (dqp W_q) added to the CAddTables' first-input gradients: dc_T = dc0 + dj[:, :R] stays in the carried cell gradient,
// dh_T = dh0 + dj[:, R:] becomes the external dL/dh of the encoder's last step, whose recurrent product is cut
struct EpiAe1wpDj {
    float *dc;        // [B][R] in: dc0, out: dc_T
    float *dh;        // [B][R] out: dh_T (the encoder's last row block of dHx)
    const float *dh0; // [B][R]
    int R;
    Drop dr;
    __device__ __forceinline__ void operator()(int, int m, int n, float v) const
    {
        const float s = dr.scale(NVQA_SITE_Q, (uint64_t)m * 2 * R + n) * v;
        if (n < R) dc[(size_t)m * R + n] += s;
        else dh[(size_t)m * R + n - R] = dh0[(size_t)m * R + n - R] + s;
    }
};

// df^ = D_V (dvp W_v)
struct EpiAe1wpDf {
    float *df;
    int I;
    Drop dr;
    __device__ __forceinline__ void operator()(int, int m, int n, float v) const
    {
        const size_t o = (size_t)m * I + n;
        df[o] = dr.scale(NVQA_SITE_V, o) * v;
    }
};

} // namespace nvqa
